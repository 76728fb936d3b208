// A map's mesh from scans and poses: range images fused into a truncated signed distance volume, and the volume's zero level set as
// triangles (ovn_tsdf_integrate, ovn_tsdf_triangles).
// Compile this file with -ffp-contract=off: both results are DEFINED as functions of float32 operations that each round on their own
// (tests/_tsdf_ref.py restates them in NumPy), and a sample is put into a pixel by the very function ovn_project uses (proj_pixel.h).
//
// Integration.  One lane per sample, a wave per run of 64 consecutive x of one (y, z) row: tsdf and weight are read once, held in
// registers through the loop over the batch's scans and written once -- 16 B of HBM traffic per sample and call, not per scan.  A
// first tiny kernel turns the poses into float32 R | o and the box of samples each scan can reach; the big kernel reads those
// records wave-uniformly and skips a scan whose box misses the wave's run.  No LDS, no atomics, no barrier; a sample has one writer.
//
// Extraction.  Marching tetrahedra over the cells in linear order, x fastest.  A workgroup owns XB consecutive cells.  Pass 1 writes one
// triangle count per workgroup, one workgroup scans those counts, pass 2 recomputes the per-cell counts, scans them inside the
// workgroup and every lane writes its cell's triangles at its offset: the order of the output is the order of the cells.
//
// Both kernels are templated on the addressing.  RING = false is the dense volume: slot (i, j, k) holds sample (i, j, k).  RING = true is
// the rolling window of ovn_tsdf_window_* (OvnRing, ovn_internal.h): a slot's lattice index comes from a compare
// and an add per axis, and every float32 operation on a sample is the dense one, so a window sample has the bits of the dense sample
// with the same lattice index.
#include <climits>

#include "ovn_internal.h"
#include "proj_pixel.h"

namespace {

// ---- integration ---------------------------------------------------------------------------------------------------------------
struct TsdfScan {
  float R[9];   // row-major rotation, float32
  float o[3];
  int lo[3];    // the samples this scan can change: lo <= (i, j, k) <= hi, lattice indices
  int hi[3];
  int ok;       // 0: a non-finite pose or an empty box
  int pad;
};

struct TsdfArgs {
  float* tsdf;
  float* weight;
  const float* range;       // (n, H, W)
  const TsdfScan* scans;    // n records, then the union of their boxes in record n
  long long n_waves;
  int nx, ny, nz, x_runs, n_scans;
  float ox, oy, oz, voxel, trunc, max_weight;
  ProjGeom gm;
  OvnRing ring;             // RING only
};

struct Int3 {
  int v[3];
};

// one thread per scan of the batch, one workgroup: the records, then the union of the boxes.  The volume holds the lattice samples
// base .. base + n - 1 on every axis (base = 0: the dense volume)
__global__ __launch_bounds__(256) void tsdf_prepare_kernel(const double* __restrict__ poses, int n_scans, int nx, int ny, int nz, Int3 base,
                                                           float ox, float oy, float oz, float voxel, float trunc, float max_range,
                                                           TsdfScan* __restrict__ scans) {
  __shared__ int ulo[3], uhi[3];
  if (threadIdx.x < 3) {
    ulo[threadIdx.x] = INT_MAX;
    uhi[threadIdx.x] = INT_MIN;
  }
  __syncthreads();
  const int dims[3] = {nx, ny, nz};
  const double org[3] = {(double)ox, (double)oy, (double)oz};
  // a sample further than this from o along ANY axis has depth > max_range + trunc > r + trunc: test 5 drops it.  One voxel and one
  // more index on each side cover the float32 roundings of the sample's coordinate and of its depth
  const double reach = ((double)max_range + (double)trunc) + (double)voxel;
  for (int s = threadIdx.x; s < n_scans; s += blockDim.x) {
    const double* P = poses + (long long)s * 16;
    TsdfScan rec;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
      for (int j = 0; j < 3; ++j) rec.R[i * 3 + j] = (float)P[i * 4 + j];
      rec.o[i] = (float)P[i * 4 + 3];
    }
    float chk = 0.0f;                              // 0 when every entry is finite, NaN otherwise
#pragma unroll
    for (int i = 0; i < 9; ++i) chk += rec.R[i] - rec.R[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) chk += rec.o[i] - rec.o[i];
    bool ok = (chk == 0.0f);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      int lo = 0, hi = -1;
      if (ok) {
        // counted from base: the clamp is the dense one
        const double l = (floor((((double)rec.o[a] - reach) - org[a]) / (double)voxel) - 1.0) - (double)base.v[a];
        const double h = (ceil((((double)rec.o[a] + reach) - org[a]) / (double)voxel) + 1.0) - (double)base.v[a];
        const double top = (double)(dims[a] - 1);
        lo = l < 0.0 ? 0 : (l > top ? dims[a] : (int)l);
        hi = h > top ? dims[a] - 1 : (h < 0.0 ? -1 : (int)h);
      }
      rec.lo[a] = base.v[a] + lo;
      rec.hi[a] = base.v[a] + hi;
      ok = ok && lo <= hi;
    }
    rec.ok = ok ? 1 : 0;
    rec.pad = 0;
    scans[s] = rec;
    if (ok) {
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        atomicMin(&ulo[a], rec.lo[a]);             // LDS, order-free: min and max
        atomicMax(&uhi[a], rec.hi[a]);
      }
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    TsdfScan u = {};
    for (int a = 0; a < 3; ++a) {
      u.lo[a] = ulo[a];
      u.hi[a] = uhi[a];
    }
    u.ok = (ulo[0] <= uhi[0]) ? 1 : 0;             // some scan had a box
    scans[n_scans] = u;
  }
}

// grid = ceil(n_waves / 4) workgroups of 4 waves; wave w owns slots (64 run .. 64 run + 63, sj, sk), w = (sk ny + sj) x_runs + run.
// RING: the run's slots are one interval of lattice x, or two when the window's seam (slot0) falls inside the run; a scan's box is
// tested against both, wave-uniformly.  The dense run is the one interval i0 .. i0 + 63
template <bool RING>
__global__ __launch_bounds__(256) void tsdf_integrate_kernel(TsdfArgs a) {
  const long long wave = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (wave >= a.n_waves) return;
  const long long row = wave / a.x_runs;
  // wave-uniform by construction; readfirstlane lets the compiler keep them, and every test on them, in scalar registers
  const int run = __builtin_amdgcn_readfirstlane((int)(wave - row * a.x_runs));
  const int sk = __builtin_amdgcn_readfirstlane((int)(row / a.ny));
  const int sj = __builtin_amdgcn_readfirstlane((int)(row - (long long)sk * a.ny));
  const int i0 = run * 64;
  int j = sj, k = sk;                            // lattice indices from here on
  int lo1 = i0, hi1 = i0 + 63;                   // the run's lattice x, first interval
  int lo2 = INT_MAX, hi2 = INT_MIN;              // and second: empty unless the seam is inside the run
  if (RING) {
    const OvnRing& r = a.ring;
    j = ovn_ring_index(sj, r.base[1], r.slot0[1], a.ny);
    k = ovn_ring_index(sk, r.base[2], r.slot0[2], a.nz);
    const int last = i0 + 63 < a.nx ? i0 + 63 : a.nx - 1;
    lo1 = ovn_ring_index(i0, r.base[0], r.slot0[0], a.nx);
    if (r.slot0[0] > i0 && r.slot0[0] <= last) {
      hi1 = r.base[0] + a.nx - 1;                // slots i0 .. slot0 - 1: the top of the window
      lo2 = r.base[0];                           // slots slot0 .. last: its bottom
      hi2 = r.base[0] + (last - r.slot0[0]);
    } else {
      hi1 = lo1 + (last - i0);
    }
  }
  const TsdfScan* __restrict__ scans = a.scans;
  {
    const TsdfScan& u = scans[a.n_scans];        // the union of the batch's boxes: most waves of a large volume end here
    if (!u.ok || j < u.lo[1] || j > u.hi[1] || k < u.lo[2] || k > u.hi[2] ||
        ((hi1 < u.lo[0] || lo1 > u.hi[0]) && (hi2 < u.lo[0] || lo2 > u.hi[0])))
      return;
  }
  const int si = i0 + (int)(threadIdx.x & 63);
  if (si >= a.nx) return;                        // nothing below crosses lanes
  const int i = RING ? ovn_ring_index(si, a.ring.base[0], a.ring.slot0[0], a.nx) : si;
  const long long idx = ((long long)sk * a.ny + sj) * a.nx + si;
  float t = a.tsdf[idx], w = a.weight[idx];
  const float px = a.ox + (float)i * a.voxel;
  const float py = a.oy + (float)j * a.voxel;
  const float pz = a.oz + (float)k * a.voxel;
  const long long HW = (long long)a.gm.H * a.gm.W;
  const float fH = (float)a.gm.H;
  for (int s = 0; s < a.n_scans; ++s) {
    const TsdfScan& sc = scans[s];
    if (!sc.ok || j < sc.lo[1] || j > sc.hi[1] || k < sc.lo[2] || k > sc.hi[2] ||
        ((hi1 < sc.lo[0] || lo1 > sc.hi[0]) && (hi2 < sc.lo[0] || lo2 > sc.hi[0])))
      continue;
    const float d0 = px - sc.o[0], d1 = py - sc.o[1], d2 = pz - sc.o[2];
    const float q0 = (sc.R[0] * d0 + sc.R[3] * d1) + sc.R[6] * d2;      // R^T d
    const float q1 = (sc.R[1] * d0 + sc.R[4] * d1) + sc.R[7] * d2;
    const float q2 = (sc.R[2] * d0 + sc.R[5] * d1) + sc.R[8] * d2;
    const float depth = point_depth(q0, q1, q2);
    if (!(depth > 0.0f)) continue;
    float yaw, pitch, fx, fy;
    point_to_subpixel(q0, q1, q2, depth, a.gm, yaw, pitch, fx, fy);
    if (!(fy >= 0.0f && fy < fH)) continue;      // outside the vertical field of view: no row to compare with (NaN included)
    const int col = (int)clamp_column(fx, a.gm);
    const int rowp = (int)floorf(fy);            // 0 .. H - 1 by the test above
    const float r = a.range[(long long)s * HW + (long long)rowp * a.gm.W + col];
    if (!(r > 0.0f && r < a.gm.max_range)) continue;
    const float sdf = r - depth;
    if (sdf < -a.trunc) continue;                // behind the surface: unseen
    const float dv = fminf(1.0f, sdf / a.trunc);
    const float w1 = w + 1.0f;
    t = (w * t + dv) / w1;
    w = fminf(w1, a.max_weight);
  }
  a.tsdf[idx] = t;
  a.weight[idx] = w;
}

// ---- extraction ----------------------------------------------------------------------------------------------------------------
constexpr int XB = 128;        // cells per workgroup, one per lane
constexpr int SCAN_T = 1024;   // threads of the one workgroup that scans the workgroup counts
constexpr int SCAN_PER = 8;    // consecutive counts per thread and step

// the six tetrahedra around the diagonal 0-7; corner c = dx + 2 dy + 4 dz.  All six have the same (positive) orientation
__device__ constexpr unsigned char TET[6][4] = {{0, 1, 3, 7}, {0, 3, 2, 7}, {0, 2, 6, 7}, {0, 6, 4, 7}, {0, 4, 5, 7}, {0, 5, 1, 7}};
// per inside mask (bit l = local vertex l has tsdf < 0): up to two triangles = six edges, four bits each, a | b << 2 for the edge
// between local vertices a and b (DESIGN.md section 29 lists them)
__device__ constexpr unsigned EDGES[16] = {0x000000u, 0x000c84u, 0x0009d1u, 0x9d8dc8u, 0x000e62u, 0xe6c64cu, 0x2e1ed1u, 0x000b73u,
                                           0x0007b3u, 0x7b4b84u, 0xb39319u, 0x0006e2u, 0x372762u, 0x000d91u, 0x0008c4u, 0x000000u};

struct ExtractArgs {
  const float* tsdf;
  const float* weight;
  float* triangles;          // (capacity, 3, 3) or NULL
  long long* wg;             // one word per workgroup: its count (pass 1), then its exclusive prefix
  long long n_cells, capacity;
  int nx, ny, nz;
  int cx, cy;                // the cells run over a box cx wide and cy deep, x fastest; dense: nx - 1, ny - 1
  int lo[3];                 // the lattice index of cell 0's low corner; dense: 0
  float ox, oy, oz, voxel, min_weight;
  OvnRing ring;              // RING only
};

// where lattice sample (i, j, k) is stored
template <bool RING>
__device__ __forceinline__ long long sample_at(const ExtractArgs& a, int i, int j, int k) {
  if (RING) {
    i = ovn_ring_slot(i, a.ring.base[0], a.ring.slot0[0], a.nx);
    j = ovn_ring_slot(j, a.ring.base[1], a.ring.slot0[1], a.ny);
    k = ovn_ring_slot(k, a.ring.base[2], a.ring.slot0[2], a.nz);
  }
  return ((long long)k * a.ny + j) * a.nx + i;
}

// exclusive prefix of v over the workgroup's XB lanes, and the workgroup's total
__device__ __forceinline__ int block_exclusive(int v, int& total) {
  __shared__ int wave_sum[XB / 64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int incl = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int up = __shfl_up(incl, d, 64);
    if (lane >= d) incl += up;
  }
  if (lane == 63) wave_sum[wv] = incl;
  __syncthreads();
  int base = 0;
  total = 0;
#pragma unroll
  for (int q = 0; q < XB / 64; ++q) {
    if (q < wv) base += wave_sum[q];
    total += wave_sum[q];
  }
  return base + incl - v;
}

template <bool WRITE, bool RING>
__global__ __launch_bounds__(XB) void tsdf_cells_kernel(ExtractArgs a) {
  const long long cell = (long long)blockIdx.x * XB + threadIdx.x;
  const int cx = a.cx, cy = a.cy;
  int count = 0, i = 0, j = 0, k = 0;   // the cell's low corner, lattice indices
  unsigned inside = 0;           // bit c: corner c has tsdf < 0
  if (cell < a.n_cells) {
    const long long rowc = cell / cx;
    i = (int)(cell - rowc * cx);
    k = (int)(rowc / cy);
    j = (int)(rowc - (long long)k * cy);
    i += a.lo[0];
    j += a.lo[1];
    k += a.lo[2];
    bool seen = true;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const long long s = sample_at<RING>(a, i + (c & 1), j + ((c >> 1) & 1), k + (c >> 2));
      seen = seen && (a.weight[s] >= a.min_weight);
      inside |= (a.tsdf[s] < 0.0f ? 1u : 0u) << c;
    }
    if (seen && inside != 0u && inside != 0xffu) {
#pragma unroll
      for (int t = 0; t < 6; ++t) {
        const unsigned m = ((inside >> TET[t][0]) & 1u) | (((inside >> TET[t][1]) & 1u) << 1) | (((inside >> TET[t][2]) & 1u) << 2) |
                           (((inside >> TET[t][3]) & 1u) << 3);
        const int p = __popc(m);
        count += (p == 2) ? 2 : ((p == 1 || p == 3) ? 1 : 0);
      }
    }
  }
  int total;
  const int before = block_exclusive(count, total);
  if (!WRITE) {
    if (threadIdx.x == 0) a.wg[blockIdx.x] = total;
    return;
  }
  if (count == 0) return;
  long long g = a.wg[blockIdx.x] + before;       // this cell's first triangle
  const float org[3] = {a.ox, a.oy, a.oz};
  for (int t = 0; t < 6; ++t) {
    const unsigned m = ((inside >> TET[t][0]) & 1u) | (((inside >> TET[t][1]) & 1u) << 1) | (((inside >> TET[t][2]) & 1u) << 2) |
                       (((inside >> TET[t][3]) & 1u) << 3);
    const int p = __popc(m);
    const int ntri = (p == 2) ? 2 : ((p == 1 || p == 3) ? 1 : 0);
    unsigned e = EDGES[m];
    for (int q = 0; q < ntri; ++q, ++g) {
      if (g >= a.capacity) return;               // ascending: nothing of this cell fits any more
      float* out = a.triangles + g * 9;
      for (int v = 0; v < 3; ++v, e >>= 4) {
        const int ca = TET[t][e & 3u], cb = TET[t][(e >> 2) & 3u];
        const int cl = ca < cb ? ca : cb, ch = ca < cb ? cb : ca;   // the corner with the smaller sample index leads
        const int il[3] = {i + (cl & 1), j + ((cl >> 1) & 1), k + (cl >> 2)};
        const int ih[3] = {i + (ch & 1), j + ((ch >> 1) & 1), k + (ch >> 2)};
        const float dl = a.tsdf[sample_at<RING>(a, il[0], il[1], il[2])];
        const float dh = a.tsdf[sample_at<RING>(a, ih[0], ih[1], ih[2])];
        const float f = dl / (dl - dh);          // the signs differ: dl - dh != 0
#pragma unroll
        for (int x = 0; x < 3; ++x) {
          const float pl = org[x] + (float)il[x] * a.voxel;
          const float ph = org[x] + (float)ih[x] * a.voxel;
          out[v * 3 + x] = pl + (ph - pl) * f;
        }
      }
    }
  }
}

// one workgroup: counts -> exclusive prefixes in place, the total to *total_out
__global__ __launch_bounds__(SCAN_T) void tsdf_scan_kernel(long long* __restrict__ wg, long long n, long long* __restrict__ total_out) {
  __shared__ long long wave_sum[SCAN_T / 64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  long long carry = 0;
  for (long long base = 0; base < n; base += (long long)SCAN_T * SCAN_PER) {
    const long long first = base + (long long)threadIdx.x * SCAN_PER;
    long long v[SCAN_PER], sum = 0;
#pragma unroll
    for (int q = 0; q < SCAN_PER; ++q) {
      v[q] = first + q < n ? wg[first + q] : 0;
      sum += v[q];
    }
    long long incl = sum;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const long long up = __shfl_up(incl, d, 64);
      if (lane >= d) incl += up;
    }
    if (lane == 63) wave_sum[wv] = incl;
    __syncthreads();
    long long before = 0, total = 0;
    for (int q = 0; q < SCAN_T / 64; ++q) {
      if (q < wv) before += wave_sum[q];
      total += wave_sum[q];
    }
    long long run = carry + before + (incl - sum);
#pragma unroll
    for (int q = 0; q < SCAN_PER; ++q) {
      if (first + q < n) wg[first + q] = run;
      run += v[q];
    }
    carry += total;
    __syncthreads();                             // wave_sum is rewritten by the next step
  }
  if (threadIdx.x == 0) *total_out = carry;
}

struct TsdfScanScratch {
  TsdfScan* scans = nullptr;
  TsdfScanScratch() = default;
  TsdfScanScratch(OvnCarver& c, size_t n) { scans = c.take<TsdfScan>(n); }
};

struct TsdfCellScratch {
  long long* wg = nullptr;
  TsdfCellScratch() = default;
  TsdfCellScratch(OvnCarver& c, size_t n) { wg = c.take<long long>(n); }
};

}  // namespace

int ovn_tsdf_integrate_forward(ovn_ctx* ctx, float* tsdf, float* weight, int nx, int ny, int nz, const double* origin, double voxel,
                               double trunc, double max_weight, const float* range, const double* poses, int n_scans, int H, int W,
                               double fov_up_deg, double fov_down_deg, double max_range, hipStream_t stream, const OvnRing* ring) {
  TsdfScanScratch sc;
  int rc = ovn_ws_layout(ctx, stream, &sc, (size_t)n_scans + 1);
  if (rc) return rc;
  scratch_overwritten(ctx);
  TsdfArgs a;
  a.tsdf = tsdf;
  a.weight = weight;
  a.range = range;
  a.scans = sc.scans;
  a.nx = nx;
  a.ny = ny;
  a.nz = nz;
  a.x_runs = (nx + 63) / 64;
  a.n_waves = (long long)a.x_runs * ny * nz;
  a.n_scans = n_scans;
  a.ox = (float)origin[0];
  a.oy = (float)origin[1];
  a.oz = (float)origin[2];
  a.voxel = (float)voxel;
  a.trunc = (float)trunc;
  a.max_weight = (float)max_weight;
  a.gm = make_geom(H, W, fov_up_deg, fov_down_deg, max_range, ctx->proj_trig);
  a.ring = ring ? *ring : OvnRing{};
  const Int3 base = {{a.ring.base[0], a.ring.base[1], a.ring.base[2]}};
  hipLaunchKernelGGL(tsdf_prepare_kernel, dim3(1), dim3(256), 0, stream, poses, n_scans, nx, ny, nz, base, a.ox, a.oy, a.oz, a.voxel,
                     a.trunc, a.gm.max_range, sc.scans);
  const long long blocks = (a.n_waves + 3) / 4;   // <= 2^31 (1/64 + 1/nx) / 4 + ny nz / 4 < 2^31
  if (ring)
    hipLaunchKernelGGL(tsdf_integrate_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, stream, a);
  else
    hipLaunchKernelGGL(tsdf_integrate_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, stream, a);
  OVN_HIP_CHECK(hipGetLastError());
  return OVN_OK;
}

int ovn_tsdf_triangles_forward(ovn_ctx* ctx, const float* tsdf, const float* weight, int nx, int ny, int nz, const double* origin,
                               double voxel, double min_weight, float* triangles, int64_t capacity, int64_t* n_triangles,
                               hipStream_t stream, const OvnRing* ring, const int* box_lo, const int* box_hi) {
  ExtractArgs a;
  a.tsdf = tsdf;
  a.weight = weight;
  a.triangles = triangles;
  a.capacity = capacity;
  a.nx = nx;
  a.ny = ny;
  a.nz = nz;
  a.ring = ring ? *ring : OvnRing{};
  int cz = nz - 1;
  a.cx = nx - 1;
  a.cy = ny - 1;
  for (int x = 0; x < 3; ++x) a.lo[x] = 0;
  if (ring) {                                    // the cells whose low corner lies in box_lo <= (I, J, K) < box_hi
    for (int x = 0; x < 3; ++x) a.lo[x] = box_lo[x];
    a.cx = box_hi[0] - box_lo[0];
    a.cy = box_hi[1] - box_lo[1];
    cz = box_hi[2] - box_lo[2];
  }
  a.n_cells = (long long)a.cx * a.cy * cz;
  a.ox = (float)origin[0];
  a.oy = (float)origin[1];
  a.oz = (float)origin[2];
  a.voxel = (float)voxel;
  a.min_weight = (float)min_weight;
  const long long n_wg = (a.n_cells + XB - 1) / XB;   // < 2^24
  TsdfCellScratch sc;
  int rc = ovn_ws_layout(ctx, stream, &sc, (size_t)(n_wg > 0 ? n_wg : 1));
  if (rc) return rc;
  scratch_overwritten(ctx);
  a.wg = sc.wg;
  const bool write = triangles && capacity > 0;
  if (ring) {                                    // an empty box has no cells: the scan alone writes the count 0
    if (n_wg > 0) hipLaunchKernelGGL((tsdf_cells_kernel<false, true>), dim3((unsigned)n_wg), dim3(XB), 0, stream, a);
    hipLaunchKernelGGL(tsdf_scan_kernel, dim3(1), dim3(SCAN_T), 0, stream, sc.wg, n_wg, reinterpret_cast<long long*>(n_triangles));
    if (write && n_wg > 0) hipLaunchKernelGGL((tsdf_cells_kernel<true, true>), dim3((unsigned)n_wg), dim3(XB), 0, stream, a);
  } else {
    hipLaunchKernelGGL((tsdf_cells_kernel<false, false>), dim3((unsigned)n_wg), dim3(XB), 0, stream, a);
    hipLaunchKernelGGL(tsdf_scan_kernel, dim3(1), dim3(SCAN_T), 0, stream, sc.wg, n_wg, reinterpret_cast<long long*>(n_triangles));
    if (write) hipLaunchKernelGGL((tsdf_cells_kernel<true, false>), dim3((unsigned)n_wg), dim3(XB), 0, stream, a);
  }
  OVN_HIP_CHECK(hipGetLastError());
  return OVN_OK;
}
