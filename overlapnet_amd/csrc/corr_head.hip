// Correlation (yaw) head of OverlapNet for gfx950, direct form, at the context's feature width W (45 <= W <= 512; 360 in the shipped
// configuration).
//
// Reference: src/two_heads/generateNet.py:327-354 -> NormalizedCorrelation2D (NormalizedCorrelation2D.py:43-109) over
// RangePadding2D(padding = W // 2) (RangePadding2D.py:31-38):
//     corr[k] = sum_{j<W} sum_{c<128} l[(k + j + W//2) mod W, c] * r[j, c],     k in [0, W)
// and the post-processing of Infer (infer.py:158): yaw = 180 - argmax_k corr[k], first maximum wins (verbatim: the bin is not
// rescaled to degrees at other widths).
//
// Direct form on the fp32 matrix cores: the Gram matrix G = l r^T (W x W, K = 128) is produced 16 query columns at a time (the last
// panel partial) with v_mfma_f32_16x16x4_f32 and immediately folded along its wrapped diagonals, corr[k] += G[(k + j + W//2) mod W, j].
// Thread k owns corr[k]; panels and the columns inside a panel are added in a fixed order, so the result (and the argmax) is
// deterministic.  One workgroup (8 waves) = one pair, each wave owning T row tiles (T = 3 up to 384 rows, else 4); the candidate
// feature volume is read from HBM exactly once.
// With a normalisation mode (ovn_set_corr_normalization) the NORM instantiation first derives both volumes' per-channel affine forms
// (ovn_corr_norm_affine, two more reads of each volume from L2) and normalises every operand as it is loaded; mode 0 launches the
// NORM = false kernel.
// LDS (dynamic): the Gram panel [W][17] floats, plus with a mode the affine forms and the block statistics (<= 86 KB at W = 512).
#include "ovn_internal.h"

namespace {

constexpr int FC = OVN_FEAT_C;
constexpr int GS_STRIDE = 17;  // floats per Gram row in LDS (16 + 1: column reads hit distinct banks)

// LDS of the normalised instantiation, after the Gram panel
struct NormLds {
  double aff[4][FC];          // m, s of L; m, s of R
  OvnNormLds<OVN_NORM_NB_MAX, FC> st;
};

__host__ __device__ inline size_t gram_bytes(int W) { return (((size_t)W * GS_STRIDE * sizeof(float)) + 15) & ~(size_t)15; }

// <3, false> (the shipped 360 columns without a mode) is held to 128 VGPRs = 4 waves per SIMD, so that two workgroups share a CU; left
// to itself the compiler takes 130 and halves the occupancy.  The other instantiations keep the 2 waves the workgroup size implies.
template <int T, bool NORM>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(T == 3 && !NORM ? 4 : 2)))
void corr_head_kernel(const float* __restrict__ feats_l, const int32_t* __restrict__ lidx, const float* __restrict__ feats_r,
                      const int32_t* __restrict__ ridx, int W, int32_t* __restrict__ yaw, float* __restrict__ corr, int norm_mode) {
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
    NormLds& nl = *reinterpret_cast<NormLds*>(reinterpret_cast<char*>(csm) + gram_bytes(W));
    ovn_corr_norm_affine(L, W, norm_mode, nl.st);
    if (tid < FC) {
      nl.aff[0][tid] = nl.st.m[tid];
      nl.aff[1][tid] = nl.st.s[tid];
    }
    __syncthreads();
    ovn_corr_norm_affine(R, W, norm_mode, nl.st);
    if (tid < FC) {
      nl.aff[2][tid] = nl.st.m[tid];
      nl.aff[3][tid] = nl.st.s[tid];
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
  const size_t lds = gram_bytes(W) + (NORM ? sizeof(NormLds) : 0);
  const size_t lds_max = gram_bytes(OVN_FEAT_W_MAX) + (NORM ? sizeof(NormLds) : 0);
  int rc = ovn_allow_dynamic_lds(reinterpret_cast<const void*>(corr_head_kernel<T, NORM>), lds_max);
  if (rc) return rc;
  hipLaunchKernelGGL((corr_head_kernel<T, NORM>), dim3(n), dim3(512), lds, stream, feats_l, lidx, feats_r, ridx, W, yaw, corr,
                     norm_mode);
  OVN_HIP_CHECK(hipGetLastError());
  return OVN_OK;
}

}  // namespace

int ovn_corr_forward(const float* feats_l, const int32_t* lidx, const float* feats_r, const int32_t* ridx, int n, int W,
                       int32_t* yaw, float* corr, hipStream_t stream, int norm_mode) {
  OVN_REQUIRE(W >= OVN_FEAT_W_MIN && W <= OVN_FEAT_W_MAX, OVN_ERR_ARG, "correlation head: width %d outside [%d, %d]", W,
              OVN_FEAT_W_MIN, OVN_FEAT_W_MAX);
  if (W <= 384)
    return norm_mode == 0 ? launch_corr<3, false>(feats_l, lidx, feats_r, ridx, n, W, yaw, corr, stream, 0)
                          : launch_corr<3, true>(feats_l, lidx, feats_r, ridx, n, W, yaw, corr, stream, norm_mode);
  return norm_mode == 0 ? launch_corr<4, false>(feats_l, lidx, feats_r, ridx, n, W, yaw, corr, stream, 0)
                        : launch_corr<4, true>(feats_l, lidx, feats_r, ridx, n, W, yaw, corr, stream, norm_mode);
}
