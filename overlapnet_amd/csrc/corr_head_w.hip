// Correlation (yaw) head of OverlapNet at a runtime feature width W (45 <= W <= 512, W != 360) for gfx950.
//
// Same formula and structure as corr_head.hip, with W in place of the fixed 360 (NormalizedCorrelation2D.py:43-109 over
// RangePadding2D(padding = W // 2)):
//     corr[k] = sum_{j<W} sum_{c<128} l[(k + j + W//2) mod W, c] * r[j, c],     k in [0, W)
// and yaw = 180 - argmax_k corr[k], first maximum wins (infer.py:158, verbatim: the bin is not rescaled to degrees).
// The Gram matrix G = l r^T (W x W, K = 128) comes off v_mfma_f32_16x16x4_f32 16 query columns at a time (the last panel partial)
// and is folded along its wrapped diagonals by thread k in a fixed order; one workgroup (8 waves) per pair, each wave owning T row
// tiles (T = 3 up to 384 rows, else 4).
// A normalisation mode (ovn_set_corr_normalization) derives both volumes' per-channel affine forms first (corr_norm_affine_w: the
// statistics of ovn_corr_norm_affine with blocks of 24 columns, the last one partial) and normalises every operand on load.
// LDS (dynamic): the Gram panel [W][17] floats, plus with a mode the affine forms and the block statistics (<= 86 KB at W = 512).
#include "ovn_internal.h"

namespace {

constexpr int FC = OVN_FEAT_C;
constexpr int GS_STRIDE = 17;  // floats per Gram row in LDS (16 + 1: column reads hit distinct banks)
constexpr int NBLK = OVN_NORM_BLK;                                           // 24 columns per partial sum
constexpr int NB_MAX = (OVN_FEAT_W_MAX + NBLK - 1) / NBLK;                   // 22

// LDS of the normalised instantiation, after the Gram panel
struct NormLdsW {
  double aff[4][FC];          // m, s of L; m, s of R
  double m[FC], s[FC];
  double part[NB_MAX][FC];
  float mn[NB_MAX][FC], mx[NB_MAX][FC];
};

// Affine form x' = RN32(((x - m) + a) s) of the 128 channels of one (W, 128) volume into L.m / L.s (ovn_corr_norm_affine's
// arithmetic: fp64 block sums in column order, then the blocks in order).  Every thread calls it; it ends with a barrier.
__device__ void corr_norm_affine_w(const float* __restrict__ X, int W, int mode, NormLdsW& L) {
  const int tid = threadIdx.x, nt = blockDim.x;
  const int nb = (W + NBLK - 1) / NBLK;
  for (int t = tid; t < nb * FC; t += nt) {   // pass 1: block sums, minima, maxima
    const int c = t % FC, b = t / FC;
    const int i1 = (b + 1) * NBLK < W ? (b + 1) * NBLK : W;
    double sm = 0.0;
    float lo = INFINITY, hi = -INFINITY;
    for (int i = b * NBLK; i < i1; ++i) {
      const float v = X[(size_t)i * FC + c];
      sm += (double)v;
      lo = fminf(lo, v);
      hi = fmaxf(hi, v);
    }
    L.part[b][c] = sm;
    L.mn[b][c] = lo;
    L.mx[b][c] = hi;
  }
  __syncthreads();
  if (tid < FC) {
    double sm = 0.0;
    float lo = INFINITY, hi = -INFINITY;
    for (int b = 0; b < nb; ++b) {
      sm += L.part[b][tid];
      lo = fminf(lo, L.mn[b][tid]);
      hi = fmaxf(hi, L.mx[b][tid]);
    }
    if (mode == 2) {
      L.m[tid] = (double)lo;
      L.s[tid] = 1.0 / (((double)hi - (double)lo) + 1e-6);
    } else {
      L.m[tid] = (mode == 3) ? sm / (double)W : 0.0;
      L.s[tid] = 0.0;
    }
  }
  __syncthreads();
  if (mode == 2) return;
  const double a = ovn_corr_norm_add(mode);
  for (int t = tid; t < nb * FC; t += nt) {   // pass 2 (euclidean, standardization): block sums of y^2
    const int c = t % FC, b = t / FC;
    const int i1 = (b + 1) * NBLK < W ? (b + 1) * NBLK : W;
    const double m = L.m[c];
    double q = 0.0;
    for (int i = b * NBLK; i < i1; ++i) {
      const double y = ((double)X[(size_t)i * FC + c] - m) + a;
      q = __builtin_fma(y, y, q);
    }
    L.part[b][c] = q;
  }
  __syncthreads();
  if (tid < FC) {
    double q = 0.0;
    for (int b = 0; b < nb; ++b) q += L.part[b][tid];
    L.s[tid] = 1.0 / sqrt(q > 1e-12 ? q : 1e-12);
  }
  __syncthreads();
}

__host__ __device__ inline size_t gram_bytes(int W) { return (((size_t)W * GS_STRIDE * sizeof(float)) + 15) & ~(size_t)15; }

template <int T, bool NORM>
__global__ __launch_bounds__(512) void corr_head_w_kernel(const float* __restrict__ feats_l, const int32_t* __restrict__ lidx,
                                                          const float* __restrict__ feats_r, const int32_t* __restrict__ ridx, int W,
                                                          int32_t* __restrict__ yaw, float* __restrict__ corr, int norm_mode) {
  extern __shared__ __attribute__((aligned(16))) float csm[];
  __shared__ float red_v[8];
  __shared__ int red_i[8];
  float* gs = csm;   // [W][17]

  const int pair = blockIdx.x;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int lrow = lane & 15;
  const int g = lane >> 4;
  const long long fe = (long long)W * FC;

  const float* L = feats_l + (long long)(lidx ? lidx[pair] : pair) * fe;
  const float* R = feats_r + (long long)(ridx ? ridx[pair] : 0) * fe;

  const double* aff = nullptr;
  double na = 0.0;
  if constexpr (NORM) {
    NormLdsW& nl = *reinterpret_cast<NormLdsW*>(reinterpret_cast<char*>(csm) + gram_bytes(W));
    corr_norm_affine_w(L, W, norm_mode, nl);
    if (tid < FC) {
      nl.aff[0][tid] = nl.m[tid];
      nl.aff[1][tid] = nl.s[tid];
    }
    __syncthreads();
    corr_norm_affine_w(R, W, norm_mode, nl);
    if (tid < FC) {
      nl.aff[2][tid] = nl.m[tid];
      nl.aff[3][tid] = nl.s[tid];
    }
    __syncthreads();
    aff = &nl.aff[0][0];
    na = ovn_corr_norm_add(norm_mode);
  }

  // A operand: rows i = 16 (T wave + t) + lrow, channels 32g..32g+31
  f32x4 lreg[T][8];
#pragma unroll
  for (int t = 0; t < T; ++t) {
    const int i = 16 * (T * wave + t) + lrow;
#pragma unroll
    for (int q = 0; q < 8; ++q)
      lreg[t][q] = (i < W) ? *reinterpret_cast<const f32x4*>(L + i * FC + 32 * g + 4 * q) : (f32x4){0.f, 0.f, 0.f, 0.f};
    if constexpr (NORM) {
      if (i < W)
#pragma unroll
        for (int q = 0; q < 8; ++q)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int c = 32 * g + 4 * q + e;
            lreg[t][q][e] = ovn_corr_norm_apply(lreg[t][q][e], aff[c], na, aff[FC + c]);
          }
    }
  }

  float partial = 0.f;
  for (int j0 = 0; j0 < W; j0 += 16) {
    // B operand: column j = j0 + lrow of r^T; columns past W in the last panel are clamped reads, never folded
    int j = j0 + lrow;
    if (j > W - 1) j = W - 1;
    f32x4 rreg[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) rreg[q] = *reinterpret_cast<const f32x4*>(R + j * FC + 32 * g + 4 * q);
    if constexpr (NORM) {
#pragma unroll
      for (int q = 0; q < 8; ++q)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int c = 32 * g + 4 * q + e;
          rreg[q][e] = ovn_corr_norm_apply(rreg[q][e], aff[2 * FC + c], na, aff[3 * FC + c]);
        }
    }

    f32x4 acc[T];
#pragma unroll
    for (int t = 0; t < T; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < 8; ++q)
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int t = 0; t < T; ++t)
          acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(lreg[t][q][e], rreg[q][e], acc[t], 0, 0, 0);

    // G tile -> LDS.  C/D: lane holds column lrow (= j - j0), rows 4g..4g+3.
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = 16 * (T * wave + t) + 4 * g + r;
        if (i < W) gs[i * GS_STRIDE + lrow] = acc[t][r];
      }
    __syncthreads();
    if (tid < W) {
      const int jn = (W - j0 < 16) ? (W - j0) : 16;
      int row = tid + j0 + W / 2;
      row -= (row >= W) ? W : 0;
      row -= (row >= W) ? W : 0;
      for (int jl = 0; jl < jn; ++jl) {
        partial += gs[row * GS_STRIDE + jl];
        ++row;
        if (row == W) row = 0;
      }
    }
    __syncthreads();
  }

  if (corr && tid < W) corr[(long long)pair * W + tid] = partial;

  // argmax with first-maximum-wins (np.argmax semantics, infer.py:158)
  float bv = (tid < W) ? partial : -INFINITY;
  int bi = (tid < W) ? tid : 0x7fffffff;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float ov = __shfl_down(bv, off, 64);
    const int oi = __shfl_down(bi, off, 64);
    if (ov > bv || (ov == bv && oi < bi)) {
      bv = ov;
      bi = oi;
    }
  }
  if (lane == 0) {
    red_v[wave] = bv;
    red_i[wave] = bi;
  }
  __syncthreads();
  if (tid == 0) {
    float v = red_v[0];
    int i = red_i[0];
    for (int w = 1; w < 8; ++w)
      if (red_v[w] > v || (red_v[w] == v && red_i[w] < i)) {
        v = red_v[w];
        i = red_i[w];
      }
    yaw[pair] = 180 - i;
  }
}

template <int T, bool NORM>
int launch_corr(const float* feats_l, const int32_t* lidx, const float* feats_r, const int32_t* ridx, int n, int W, int32_t* yaw,
                float* corr, hipStream_t stream, int norm_mode) {
  const size_t lds = gram_bytes(W) + (NORM ? sizeof(NormLdsW) : 0);
  const size_t lds_max = gram_bytes(OVN_FEAT_W_MAX) + (NORM ? sizeof(NormLdsW) : 0);
  int rc = ovn_allow_dynamic_lds(reinterpret_cast<const void*>(corr_head_w_kernel<T, NORM>), lds_max);
  if (rc) return rc;
  hipLaunchKernelGGL((corr_head_w_kernel<T, NORM>), dim3(n), dim3(512), lds, stream, feats_l, lidx, feats_r, ridx, W, yaw, corr,
                     norm_mode);
  OVN_HIP_CHECK(hipGetLastError());
  return OVN_OK;
}

}  // namespace

int ovn_corr_w_forward(const float* feats_l, const int32_t* lidx, const float* feats_r, const int32_t* ridx, int n, int W,
                       int32_t* yaw, float* corr, hipStream_t stream, int norm_mode) {
  OVN_REQUIRE(W >= OVN_FEAT_W_MIN && W <= OVN_FEAT_W_MAX, OVN_ERR_ARG, "correlation head: width %d outside [%d, %d]", W,
              OVN_FEAT_W_MIN, OVN_FEAT_W_MAX);
  if (W <= 384)
    return norm_mode == 0 ? launch_corr<3, false>(feats_l, lidx, feats_r, ridx, n, W, yaw, corr, stream, 0)
                          : launch_corr<3, true>(feats_l, lidx, feats_r, ridx, n, W, yaw, corr, stream, norm_mode);
  return norm_mode == 0 ? launch_corr<4, false>(feats_l, lidx, feats_r, ridx, n, W, yaw, corr, stream, 0)
                        : launch_corr<4, true>(feats_l, lidx, feats_r, ridx, n, W, yaw, corr, stream, norm_mode);
}
