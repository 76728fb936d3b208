// Gradients of both heads' losses with respect to the feature volumes (ovn_heads_feature_grad), fp32, for gfx950, at any conv1size s
// and any feature width W.  Notation: G = W // s, R = s G, hp = W // 2.  Outputs are per pair: row p of dfeat_l / dfeat_r is the
// gradient reaching the volume pair p read; no kernel here sums over pairs, so there are no atomics and no pool.
//
// Overlap part (after ovn_delta_head_grad_run has left dO1 (pairs, W, G, 64) of a chunk in scratch):
//   E_p[i, s jb + dj, c] = sum_{o < 64} dO1_p[i, jb, o] W1[dj, c, o]                (W1 as registered: negateDiffs needs no case)
//   dL/dl_p[i, c] =   sum_{j < R} sgn(l_p[i, c] - r_p[j, c]) E_p[i, j, c]
//   dL/dr_p[j, c] = - sum_{i < R} sgn(l_p[i, c] - r_p[j, c]) E_p[i, j, c]           sgn(0) = 0; rows >= R get nothing
// Both walks form a 16 rows i x 16 channels c tile of E for ONE column j on v_mfma_f32_16x16x4_f32 (K = the 64 outputs o, sixteen
// MFMAs, two accumulators), multiply it by the sign formed in registers from l and r and reduce it at once: E never goes to memory.
//   delta_dl_kernel  workgroup = (16 rows i, pair), wave = 16 channels; the wave walks all R columns.  A = dO1 (held over the s taps
//                    of a column group), B = W1[dj].  A lane owns 4 rows x 1 channel of dl: no cross-lane sum.
//   delta_dr_kernel  workgroup = (column j, pair), wave = 16 channels; the wave walks the rows in tiles of 16.  B = W1[dj] stays in
//                    registers for the whole walk.  A lane sums its 4 rows per tile; the four row quarters of the wave join at the end.
// The k index of the MFMAs is the permutation o = 16 t + 4 (lane >> 4) + e of step 4 t + e, the same for A and B, so that both
// operands are 16-byte loads.  Sums: the MFMA result (64 terms) and the signed sum over at most one column group (dl: s terms) or one
// row tile (dr: 4 terms per lane) are fp32; the groups / tiles join in an fp64 running sum that is rounded once.
// Edges: 128 s is a multiple of 16; rows i >= R of a tile read row R - 1 and their A operand is zeroed by a select (EXEC stays full
// around the MFMAs), so their E is 0; stores are guarded by i < R.  The caller zero-fills dfeat_l / dfeat_r first.
//
// Yaw part (NormalizedCorrelation2D normalize = 'none' + RangePadding2D, weighted_cross_entropy_with_logits with pos_weight = W):
//   z_p[k] = sum_{j < W, c} l_p[(k + j + hp) mod W, c] r_p[j, c]                                 corr_fwd_kernel, fp64 sums, rounded once
//   q_p[k] = [k == bin_p and 0 <= bin_p < W and t_p > min_overlap_for_angle],  m = 1 + (W - 1) q
//   loss   = (1 - q) z + m (log1p(exp(-|z|)) + max(-z, 0)),   g_p[k] = yaw_scale / (n W) ((1 - q) - m sigmoid(-z))     yaw_loss_kernel, fp64
//   dL/dr_p[j, c] += sum_k g_p[k] l_p[(k + j + hp) mod W, c],   dL/dl_p[i, c] += sum_k g_p[k] r_p[(i - k - hp) mod W, c]   yaw_grad_kernel, fp64
// The bin is only compared with k, never used as an index.  The loss: per pair an fp64 tree over k, rounded to fp32; the pairs of
// a pair block are added in order, the pair blocks in order onto the running sum (yaw_loss_reduce_kernel), as the overlap loss is.
//
// Bounds.  l / r rows: min(i, R - 1) < W, j < R <= W, indices taken mod W; dO1 rows min(i, R - 1); W1 taps dj < s; every store is
// guarded by its row (< R or < W) and its pair is the block index (< pairs of the chunk).
// Under ovn_profile_begin the two Delta kernels report as class 8 (with the c_conv1 weight gradient), the yaw kernels as class 1.
#include "ovn_internal.h"

namespace {

constexpr int FC = OVN_FEAT_C;    // 128
constexpr int O1 = OVN_C1_OUT;    // 64
constexpr int PB = OVN_GRAD_PAIR_BLOCK;

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }

__device__ __forceinline__ float sgnf(float a, float b) { return a > b ? 1.f : (a < b ? -1.f : 0.f); }

// E tile of one column: sum over the 64 outputs, two accumulators (the 16x16x4 MFMA's dependent latency is above its issue interval)
__device__ __forceinline__ f32x4 e_tile(const f32x4 (&a)[4], const f32x4 (&b)[4]) {
  f32x4 e0 = {0.f, 0.f, 0.f, 0.f}, e1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int t = 0; t < 4; t += 2) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      e0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t][e], b[t][e], e0, 0, 0, 0);
      e1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t + 1][e], b[t + 1][e], e1, 0, 0, 0);
    }
  }
  return e0 + e1;
}

// MFMA 16x16x4: A[m = lane & 15][k = lane >> 4] = dO1[i0 + m][jb][o(k)], B[k][n = lane & 15] = W1[dj][c0 + n][o(k)];
// D: lane holds channel n = lane & 15, rows m = 4 (lane >> 4) + j
__global__ __launch_bounds__(512) void delta_dl_kernel(const float* __restrict__ feats_l, const int32_t* __restrict__ lidx,
                                                       const float* __restrict__ feats_r, const int32_t* __restrict__ ridx,
                                                       const float* __restrict__ dO1, const float* __restrict__ w1, int s, int G, int W,
                                                       float* __restrict__ dl) {
  const int p = blockIdx.y, i0 = 16 * (int)blockIdx.x;
  const int lane = (int)(threadIdx.x & 63), c = 16 * (int)(threadIdx.x >> 6) + (lane & 15);
  const int m = lane & 15, kq = lane >> 4;
  const int R = s * G;
  const float* L = feats_l + (size_t)(lidx ? lidx[p] : p) * W * FC + c;
  const float* Rv = feats_r + (size_t)(ridx ? ridx[p] : 0) * W * FC + c;
  const bool oka = i0 + m < R;
  const int ia = oka ? i0 + m : R - 1;
  const float* Da = dO1 + ((size_t)p * W + ia) * G * O1 + 4 * kq;
  const float* Wb = w1 + (size_t)c * O1 + 4 * kq;
  float lv[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int i = i0 + 4 * kq + j;
    lv[j] = L[(size_t)(i < R ? i : R - 1) * FC];
  }
  double sum[4] = {0.0, 0.0, 0.0, 0.0};
  for (int jb = 0; jb < G; ++jb) {
    f32x4 a[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const f32x4 v = ld4(Da + (size_t)jb * O1 + 16 * t);
      a[t] = oka ? v : f32x4{0.f, 0.f, 0.f, 0.f};
    }
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int dj = 0; dj < s; ++dj) {
      f32x4 b[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) b[t] = ld4(Wb + (size_t)dj * FC * O1 + 16 * t);
      const float rv = Rv[(size_t)(s * jb + dj) * FC];
      const f32x4 e = e_tile(a, b);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = fmaf(sgnf(lv[j], rv), e[j], acc[j]);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) sum[j] += (double)acc[j];
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int i = i0 + 4 * kq + j;
    if (i < R) dl[((size_t)p * W + i) * FC + c] = (float)sum[j];
  }
}

__global__ __launch_bounds__(512) void delta_dr_kernel(const float* __restrict__ feats_l, const int32_t* __restrict__ lidx,
                                                       const float* __restrict__ feats_r, const int32_t* __restrict__ ridx,
                                                       const float* __restrict__ dO1, const float* __restrict__ w1, int s, int G, int W,
                                                       float* __restrict__ dr) {
  const int p = blockIdx.y, jcol = (int)blockIdx.x;
  const int jb = jcol / s, dj = jcol - jb * s;
  const int lane = (int)(threadIdx.x & 63), c = 16 * (int)(threadIdx.x >> 6) + (lane & 15);
  const int m = lane & 15, kq = lane >> 4;
  const int R = s * G;
  const float* L = feats_l + (size_t)(lidx ? lidx[p] : p) * W * FC + c;
  const float rv = feats_r[(size_t)(ridx ? ridx[p] : 0) * W * FC + (size_t)jcol * FC + c];
  const float* D = dO1 + ((size_t)p * W * G + jb) * O1 + 4 * kq;
  f32x4 b[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) b[t] = ld4(w1 + ((size_t)dj * FC + c) * O1 + 4 * kq + 16 * t);
  double sum = 0.0;
  for (int i0 = 0; i0 < R; i0 += 16) {
    const bool oka = i0 + m < R;
    const int ia = oka ? i0 + m : R - 1;
    f32x4 a[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const f32x4 v = ld4(D + (size_t)ia * G * O1 + 16 * t);
      a[t] = oka ? v : f32x4{0.f, 0.f, 0.f, 0.f};
    }
    float lv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int i = i0 + 4 * kq + j;
      lv[j] = L[(size_t)(i < R ? i : R - 1) * FC];
    }
    const f32x4 e = e_tile(a, b);
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) acc = fmaf(sgnf(lv[j], rv), e[j], acc);   // rows >= R: e = 0
    sum += (double)acc;
  }
  // the four row quarters (lanes n, n + 16, n + 32, n + 48): (q0 + q1) + (q2 + q3) on every lane
  sum += __shfl_xor(sum, 16);
  sum += __shfl_xor(sum, 32);
  if (kq == 0) dr[((size_t)p * W + jcol) * FC + c] = (float)(-sum);
}

// z[p][k]: wave = 4 consecutive k, lane = channels 2 lane, 2 lane + 1; products of two floats are exact in fp64
__global__ __launch_bounds__(256) void corr_fwd_kernel(const float* __restrict__ feats_l, const int32_t* __restrict__ lidx,
                                                       const float* __restrict__ feats_r, const int32_t* __restrict__ ridx, int W,
                                                       float* __restrict__ z) {
  const int p = blockIdx.y;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = (int)(threadIdx.x & 63);
  const int k0 = 16 * (int)blockIdx.x + 4 * wave;
  if (k0 >= W) return;
  const float* L = feats_l + (size_t)(lidx ? lidx[p] : p) * W * FC + 2 * lane;
  const float* Rv = feats_r + (size_t)(ridx ? ridx[p] : 0) * W * FC + 2 * lane;
  int row[4];
  double acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int k = k0 + t < W ? k0 + t : W - 1;
    row[t] = (k + W / 2) % W;
    acc[t] = 0.0;
  }
  for (int j = 0; j < W; ++j) {
    const float2 rv = *reinterpret_cast<const float2*>(Rv + (size_t)j * FC);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const float2 lv = *reinterpret_cast<const float2*>(L + (size_t)row[t] * FC);
      acc[t] = fma((double)lv.x, (double)rv.x, acc[t]);
      acc[t] = fma((double)lv.y, (double)rv.y, acc[t]);
      row[t] = row[t] + 1 == W ? 0 : row[t] + 1;
    }
  }
#pragma unroll
  for (int t = 0; t < 4; ++t) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc[t] += __shfl_xor(acc[t], off);
    if (lane == 0 && k0 + t < W) z[(size_t)p * W + k0 + t] = (float)acc[t];
  }
}

// workgroup = pair: g[p][k] (fp64) and the pair's loss term (fp64 tree over k, rounded once)
__global__ __launch_bounds__(256) void yaw_loss_kernel(const float* __restrict__ z, const float* __restrict__ target,
                                                       const int32_t* __restrict__ bins, int W, float thr, double coef,
                                                       double* __restrict__ g, float* __restrict__ pair_loss) {
  __shared__ double red[256];
  const int p = blockIdx.x;
  const int bin = bins[p];
  const bool pos = bin >= 0 && bin < W && target[p] > thr;
  double local = 0.0;
  for (int k = threadIdx.x; k < W; k += 256) {
    const double zz = (double)z[(size_t)p * W + k];
    const bool q = pos && k == bin;
    const double mw = q ? (double)W : 1.0;
    const double sp = log1p(exp(-fabs(zz))) + fmax(-zz, 0.0);
    const double sig = 1.0 / (1.0 + exp(zz));            // sigmoid(-z)
    local += (q ? 0.0 : zz) + mw * sp;
    g[(size_t)p * W + k] = coef * ((q ? 0.0 : 1.0) - mw * sig);
  }
  red[threadIdx.x] = local;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) pair_loss[p] = (float)(coef * red[0]);
}

// one thread: running sum += the pair blocks' sums in order, pairs in order inside a block
__global__ void yaw_loss_reduce_kernel(const float* __restrict__ pair_loss, int np, int first, float* __restrict__ loss) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  float acc = first ? 0.f : *loss;
  for (int b = 0; b * PB < np; ++b) {
    float sb = 0.f;
    for (int q = 0; q < PB && b * PB + q < np; ++q) sb += pair_loss[b * PB + q];
    acc += sb;
  }
  *loss = acc;
}

// workgroup = (8 rows, pair, direction), thread = (4 rows, channel); direction 0: dr += sum_k g[k] l[(k + row + hp) mod W],
// direction 1: dl += sum_k g[k] r[(row - k - hp) mod W]; fp64 sums joined with the overlap part and rounded once
__global__ __launch_bounds__(256) void yaw_grad_kernel(const float* __restrict__ feats_l, const int32_t* __restrict__ lidx,
                                                       const float* __restrict__ feats_r, const int32_t* __restrict__ ridx,
                                                       const double* __restrict__ g, int W, float* __restrict__ dl, float* __restrict__ dr) {
  extern __shared__ double gs[];
  const int p = blockIdx.y, dir = blockIdx.z;
  for (int k = threadIdx.x; k < W; k += 256) gs[k] = g[(size_t)p * W + k];
  __syncthreads();
  const int c = (int)(threadIdx.x & 127), row0 = 8 * (int)blockIdx.x + 4 * (int)(threadIdx.x >> 7);
  const float* src = (dir == 0 ? feats_l + (size_t)(lidx ? lidx[p] : p) * W * FC : feats_r + (size_t)(ridx ? ridx[p] : 0) * W * FC) + c;
  const int hp = W / 2;
  int idx[4];
  double acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int row = row0 + t < W ? row0 + t : W - 1;
    idx[t] = dir == 0 ? (row + hp) % W : (row - hp + W) % W;
    acc[t] = 0.0;
  }
  for (int k = 0; k < W; ++k) {
    const double gk = gs[k];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      acc[t] = fma(gk, (double)src[(size_t)idx[t] * FC], acc[t]);
      if (dir == 0) idx[t] = idx[t] + 1 == W ? 0 : idx[t] + 1;
      else idx[t] = idx[t] == 0 ? W - 1 : idx[t] - 1;
    }
  }
  float* out = (dir == 0 ? dr : dl) + (size_t)p * W * FC + c;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int row = row0 + t;
    if (row < W) out[(size_t)row * FC] = (float)((double)out[(size_t)row * FC] + acc[t]);
  }
}

// Scratch of ovn_yaw_grad_run for chunks of up to cmax pairs: dL/d(logits) in fp64 | per-pair losses | the logits, unless the caller
// takes them
struct YawGradScratch {
  double* g = nullptr;
  float *pl = nullptr, *zbuf = nullptr;
  YawGradScratch() = default;
  YawGradScratch(OvnCarver& c, size_t cmax, int FW, bool own_logits) {
    g = c.take<double>(cmax * FW);
    pl = c.take<float>(cmax);
    zbuf = c.take<float>(own_logits ? cmax * FW : 0);
  }
};

}  // namespace

int ovn_delta_data_grad(ovn_ctx* ctx, int FW, const float* feats_l, const int32_t* lidx, const float* feats_r, const int32_t* ridx,
                        const float* dO1, int np, float* dfeat_l, float* dfeat_r, hipStream_t stream) {
  const int s = ctx->head_s, G = ctx->head_g, R = s * G;
  OvnProfScope ps(ctx, OVN_K_DELTA_PREP, stream);
  hipLaunchKernelGGL(delta_dl_kernel, dim3((unsigned)((R + 15) / 16), (unsigned)np), dim3(512), 0, stream, feats_l, lidx, feats_r, ridx,
                     dO1, ctx->head.w1raw, s, G, FW, dfeat_l);
  hipLaunchKernelGGL(delta_dr_kernel, dim3((unsigned)R, (unsigned)np), dim3(512), 0, stream, feats_l, lidx, feats_r, ridx, dO1,
                     ctx->head.w1raw, s, G, FW, dfeat_r);
  OVN_HIP_CHECK(hipGetLastError());
  return OVN_OK;
}

int ovn_yaw_grad_run(ovn_ctx* ctx, int FW, const float* feats_l, const int32_t* lidx, const float* feats_r, const int32_t* ridx,
                     int64_t n, const float* target, const int32_t* yaw_bin, float yaw_scale, float thr, float* dfeat_l, float* dfeat_r,
                     float* loss_yaw, float* corr, hipStream_t stream) {
  const int64_t chunk = 4096;                       // whole pair blocks; the grids' y extent
  const int64_t cmax = n < chunk ? n : chunk;
  YawGradScratch sc;
  int rc = ovn_ws_layout(ctx, stream, &sc, (size_t)cmax, FW, corr == nullptr);
  if (rc) return rc;
  scratch_overwritten(ctx);
  double* g = sc.g;
  float *pl = sc.pl, *zbuf = sc.zbuf;
  const double coef = (double)yaw_scale / ((double)n * (double)FW);
  const size_t feat_elems = (size_t)FW * FC;
  for (int64_t p0 = 0; p0 < n; p0 += chunk) {
    const int np = (int)((n - p0 < chunk) ? (n - p0) : chunk);
    const float* fl = lidx ? feats_l : feats_l + (size_t)p0 * feat_elems;
    const int32_t* li = lidx ? lidx + p0 : nullptr;
    const int32_t* ri = ridx ? ridx + p0 : nullptr;
    float* z = corr ? corr + (size_t)p0 * FW : zbuf;
    OvnProfScope ps(ctx, OVN_K_CORR, stream);
    hipLaunchKernelGGL(corr_fwd_kernel, dim3((unsigned)((FW + 15) / 16), (unsigned)np), dim3(256), 0, stream, fl, li, feats_r, ri, FW, z);
    if (!yaw_bin) {                                 // the logits alone
      OVN_HIP_CHECK(hipGetLastError());
      continue;
    }
    hipLaunchKernelGGL(yaw_loss_kernel, dim3((unsigned)np), dim3(256), 0, stream, z, target + p0, yaw_bin + p0, FW, thr, coef, g, pl);
    hipLaunchKernelGGL(yaw_loss_reduce_kernel, dim3(1), dim3(64), 0, stream, pl, np, p0 == 0 ? 1 : 0, loss_yaw);
    hipLaunchKernelGGL(yaw_grad_kernel, dim3((unsigned)((FW + 7) / 8), (unsigned)np, 2), dim3(256), (size_t)FW * sizeof(double), stream,
                       fl, li, feats_r, ri, g, FW, dfeat_l + (size_t)p0 * feat_elems, dfeat_r + (size_t)p0 * feat_elems);
    OVN_HIP_CHECK(hipGetLastError());
  }
  return OVN_OK;
}
