// Delta (overlap) head of OverlapNet for gfx950 at the context's feature width W (45 <= W <= 512; 360 in the shipped configuration)
// with conv1size 15: DeltaLayer + c_conv1 + c_conv2 fused in one kernel (exact fp32 on v_mfma_f32_16x16x4_f32), c_conv3 on the
// generic conv kernel of conv_f32.hip, and the Dense(1) + sigmoid tail.
//
// Reference: src/two_heads/generateNet.py:15-61 (DeltaLayer) and :64-116 (head).
//   diff[i,j,c] = |L[i,c] - R[j,c]|                       (W x W x 128 per pair, 66 MB at 360 in the reference)
//   o1[i,jb,o]  = b1[o] + sum_{dj<15,c} diff[i,15jb+dj,c] * W1[dj,c,o]         c_conv1, linear
//   o2[ib,jb,p] = relu(b2[p] + sum_{di<15,o} o1[15ib+di,jb,o] * W2[di,o,p])    c_conv2
// The diff tensor is never materialised: each lane keeps its slice of L in registers for the whole pair and forms |L - R| on the
// fly as the A operand of the MFMA.
//
// G = W // 15 column groups ('valid', stride 15: the last W - 15 G columns of r are never read) and only the rows i < 15 G of l
// feed c_conv2 (its 'valid' stride (15, 1) drops the rest), so the contraction runs over R = 15 G rows (G = 24, R = 360 at W = 360).
// One workgroup (8 waves) = one pair.  For each column group jb:
//   GEMM1  (R x 1920) x (1920 x 64): wave w owns row tiles T w .. T w + T - 1 (T = 3 for R <= 384, else 4), all 64 outputs.
//          K = (dj, c) is walked dj-major; within a dj, lane group g = lane>>4 covers channels 32g..32g+31, so a lane needs exactly
//          L[i, 32g..32g+31] (32 registers per row tile) and the matching R row comes from LDS as a broadcast ds_read_b128.  W1 is
//          pre-permuted to that order.  Rows >= R (zero-padded tiles) are computed and dropped before o1 reaches LDS.
//   o1 (+b1) goes to LDS as the [G][964] A matrix of GEMM2 (row ib = 15 consecutive i rows): (G * 964 + 15 * 128) * 4 B, 100,224 B at
//          G = 24 and 138,784 B at G = 34.
//   GEMM2  (G x 960) x (960 x 128): wave w owns output tile w (16 channels) for all MT = ceil(G / 16) row tiles; padding rows
//          (>= G) are clamped reads and never stored.  + b2, ReLU, store o2.
// Every output element is summed in one K order whatever the width and the tile shape: two widths give the same o2 bits on the rows
// and columns both read.
#include "ovn_internal.h"

namespace {

constexpr int FC = OVN_FEAT_C;        // 128
constexpr int S = OVN_S;              // 15
constexpr int O1 = OVN_C1_OUT;        // 64
constexpr int O2 = OVN_C2_OUT;        // 128
constexpr int K2 = S * O1;            // 960
constexpr int O1S_STRIDE = K2 + 4;    // 964 floats: odd number of 16-B slots -> conflict-free b128 rows
constexpr int G_MAX = OVN_FEAT_W_MAX / S;   // 34

// W1p[dj][sq][nt][lane][e] = W1[dj][c = 32*(lane>>4) + 4*sq + e][o = 16*nt + (lane&15)]
__global__ void delta_prep_w1_kernel(const float* __restrict__ w1, float* __restrict__ w1p) {
  const int total = S * 8 * 4 * 64 * 4;
  for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gridDim.x * blockDim.x) {
    const int e = idx & 3;
    const int lane = (idx >> 2) & 63;
    const int nt = (idx >> 8) & 3;
    const int sq = (idx >> 10) & 7;
    const int dj = idx >> 13;
    const int c = 32 * (lane >> 4) + 4 * sq + e;
    const int o = 16 * nt + (lane & 15);
    w1p[idx] = w1[(dj * FC + c) * O1 + o];  // Keras (1,15,128,64) flattened
  }
}

template <int T, int MT>
__global__ __launch_bounds__(512) void delta_c12_kernel(const float* __restrict__ feats_l, const int32_t* __restrict__ lidx,
                                                        const float* __restrict__ feats_r, const int32_t* __restrict__ ridx,
                                                        const float* __restrict__ w1p, const float* __restrict__ b1,
                                                        const float* __restrict__ w2p, const float* __restrict__ b2, int W,
                                                        float* __restrict__ o2) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int G = W / S;
  const int R = G * S;                   // rows of l that reach c_conv2
  float* o1s = smem;                     // [G][964]
  float* rs = smem + G * O1S_STRIDE;     // [15][128]

  const int pair = blockIdx.x;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int lrow = lane & 15;
  const int g = lane >> 4;
  const long long fe = (long long)W * FC;

  const float* L = feats_l + (long long)(lidx ? lidx[pair] : pair) * fe;
  const float* Rv = feats_r + (long long)(ridx ? ridx[pair] : 0) * fe;

  // this lane's slice of L: rows 16 (T wave + t) + lrow, channels 32g..32g+31
  f32x4 lreg[T][8];
#pragma unroll
  for (int t = 0; t < T; ++t) {
    const int i = 16 * (T * wave + t) + lrow;
#pragma unroll
    for (int q = 0; q < 8; ++q)
      lreg[t][q] = (i < R) ? *reinterpret_cast<const f32x4*>(L + i * FC + 32 * g + 4 * q) : (f32x4){0.f, 0.f, 0.f, 0.f};
  }

  for (int jb = 0; jb < G; ++jb) {
    __syncthreads();  // previous group's GEMM2 has finished reading o1s / rs
    if (tid < S * FC / 4)
      *reinterpret_cast<f32x4*>(rs + 4 * tid) = *reinterpret_cast<const f32x4*>(Rv + jb * S * FC + 4 * tid);
    __syncthreads();

    // T = 4: the 64 outputs in two passes of 32 (acc[4][4] beside the 128 registers of L would spill); same K order per output
    constexpr int NH = T > 3 ? 2 : 1;
    constexpr int NTH = 4 / NH;
#pragma unroll 1
    for (int h = 0; h < NH; ++h) {
    f32x4 acc[T][NTH];
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
      for (int nt = 0; nt < NTH; ++nt) acc[t][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};

    for (int dj = 0; dj < S; ++dj) {
      const float* wrow = w1p + dj * 8192 + lane * 4;
      const float* rrow = rs + dj * FC + 32 * g;
#pragma unroll
      for (int sq = 0; sq < 8; ++sq) {
        const f32x4 rv = *reinterpret_cast<const f32x4*>(rrow + 4 * sq);
        f32x4 bw[NTH];
#pragma unroll
        for (int nt = 0; nt < NTH; ++nt) bw[nt] = *reinterpret_cast<const f32x4*>(wrow + (sq * 4 + NTH * h + nt) * 256);
        f32x4 d[T];
#pragma unroll
        for (int t = 0; t < T; ++t) {
          const f32x4 lv = lreg[t][sq];
          d[t][0] = fabsf(lv[0] - rv[0]);
          d[t][1] = fabsf(lv[1] - rv[1]);
          d[t][2] = fabsf(lv[2] - rv[2]);
          d[t][3] = fabsf(lv[3] - rv[3]);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int t = 0; t < T; ++t)
#pragma unroll
            for (int nt = 0; nt < NTH; ++nt)
              acc[t][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(d[t][e], bw[nt][e], acc[t][nt], 0, 0, 0);
      }
    }

    // o1 (+ bias) -> LDS in GEMM2's A layout.  C/D: lane holds column lrow, rows 4g..4g+3 of the tile; rows >= R are dropped.
#pragma unroll
    for (int nt = 0; nt < NTH; ++nt) {
      const int o = 16 * (NTH * h + nt) + lrow;
      const float bv = b1[o];
#pragma unroll
      for (int t = 0; t < T; ++t) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int i = 16 * (T * wave + t) + 4 * g + r;
          if (i < R) {
            const int ib = i / S;
            const int di = i - ib * S;
            o1s[ib * O1S_STRIDE + di * O1 + o] = acc[t][nt][r] + bv;
          }
        }
      }
    }
    }
    __syncthreads();

    // GEMM2: wave -> n-tile `wave` (channels 16 wave ..), all MT m-tiles
    {
      const float* arow[MT];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        int ib = 16 * mt + lrow;
        if (ib > G - 1) ib = G - 1;    // padding rows of the last m-tile: clamped reads, never stored
        arow[mt] = o1s + ib * O1S_STRIDE + 4 * g;
      }
      const float* wcol = w2p + wave * 256 + lane * 4;
      f32x4 acc2[MT];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) acc2[mt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
      for (int kc = 0; kc < K2 / 16; ++kc) {
        const f32x4 bv = *reinterpret_cast<const f32x4*>(wcol + kc * (8 * 256));
        f32x4 av[MT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) av[mt] = *reinterpret_cast<const f32x4*>(arow[mt] + 16 * kc);
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) acc2[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mt][e], bv[e], acc2[mt], 0, 0, 0);
      }
      const int p = 16 * wave + lrow;
      const float bv = b2[p];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int ib2 = 16 * mt + 4 * g + r;
          if (ib2 < G) o2[(((long long)pair * G + ib2) * G + jb) * O2 + p] = fmaxf(acc2[mt][r] + bv, 0.0f);
        }
    }
  }
}

template <int T, int MT>
int launch_c12(const ovn_ctx* ctx, const float* feats_l, const int32_t* lidx, const float* feats_r, const int32_t* ridx, int n, int W,
               float* o2, hipStream_t stream) {
  const int G = W / S;
  const size_t lds = ((size_t)G * O1S_STRIDE + (size_t)S * FC) * sizeof(float);
  const size_t lds_max = ((size_t)G_MAX * O1S_STRIDE + (size_t)S * FC) * sizeof(float);
  int rc = ovn_allow_dynamic_lds(reinterpret_cast<const void*>(delta_c12_kernel<T, MT>), lds_max);
  if (rc) return rc;
  hipLaunchKernelGGL((delta_c12_kernel<T, MT>), dim3(n), dim3(512), lds, stream, feats_l, lidx, feats_r, ridx, ctx->head.w1p, ctx->head.b1,
                     ctx->head.c2.wp, ctx->head.c2.bias, W, o2);
  OVN_HIP_CHECK(hipGetLastError());
  return OVN_OK;
}

// logit[n] = bd + <o3[n,:], wd>, overlap = sigmoid(logit) for a Dense input of `dense_in` floats (a multiple of 4); Flatten order
// (H, W, C) == o3's NHWC layout (generateNet.py:112-114).  One workgroup per pair, fixed reduction order.
__global__ __launch_bounds__(256) void dense_sigmoid_kernel(const float* __restrict__ o3, const float* __restrict__ wd,
                                                            const float* __restrict__ bd, long long dense_in,
                                                            float* __restrict__ overlap, float* __restrict__ logit) {
  __shared__ float red[4];
  const int n = blockIdx.x;
  const f32x4* x = reinterpret_cast<const f32x4*>(o3 + (long long)n * dense_in);
  const f32x4* w = reinterpret_cast<const f32x4*>(wd);
  float s = 0.f;
  for (long long i = threadIdx.x; i < dense_in / 4; i += 256) {
    const f32x4 a = x[i];
    const f32x4 b = w[i];
    s += (a[0] * b[0] + a[1] * b[1]) + (a[2] * b[2] + a[3] * b[3]);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    const float z = ((red[0] + red[1]) + (red[2] + red[3])) + bd[0];
    if (logit) logit[n] = z;
    overlap[n] = 1.0f / (1.0f + expf(-z));
  }
}

}  // namespace

int ovn_delta_prepare_w1(OvnHeadWeights* hw, const float* c1_kernel_dev, hipStream_t stream) {
  const size_t elems = (size_t)S * FC * O1;
  OVN_HIP_CHECK(hipMalloc((void**)&hw->w1p, elems * sizeof(float)));
  hipLaunchKernelGGL(delta_prep_w1_kernel, dim3(120), dim3(256), 0, stream, c1_kernel_dev, hw->w1p);
  OVN_HIP_CHECK(hipGetLastError());
  return OVN_OK;
}

OvnDeltaF32Scratch::OvnDeltaF32Scratch(OvnCarver& c, int64_t n, int G, bool split) {
  o2 = c.take<float>((size_t)n * G * G * OVN_C2_OUT);
  o3 = c.take<float>((size_t)n * (G - 2) * (G - 2) * OVN_C3_OUT);
  scales = c.take<char>(split ? (size_t)n * ovn_delta_w_split_pair_bytes() : 0);
}

// Bytes of scratch per pair, unaligned: o2 (G, G, 128) | o3 (G - 2, G - 2, 256) | the split route's per-pair scales
size_t ovn_delta_pair_bytes(int G) {
  return ((size_t)G * G * OVN_C2_OUT + (size_t)(G - 2) * (G - 2) * OVN_C3_OUT) * sizeof(float) + ovn_delta_w_split_pair_bytes();
}

// The whole Delta head for n pairs at the context's feature width (360 before ovn_finalize), conv1size 15, in a scratch laid out for
// at least n pairs (with its scales when the split route is on).
// DeltaLayer + c_conv1 + c_conv2 run exact fp32 here, or in f16x3 arithmetic (delta_head_w_f16x3.hip) when the context asks for
// it (head mode 1 with ovn_set_head_width_split); c_conv3 and Dense are the same fp32 kernels either way.
int ovn_delta_forward(ovn_ctx* ctx, const float* feats_l, const int32_t* lidx, const float* feats_r, const int32_t* ridx, int n,
                      const OvnDeltaF32Scratch& scratch, float* overlap, float* logit, hipStream_t stream) {
  const int W = ctx->finalized ? ctx->feat_w : OVN_FEAT_W, G = W / S, R = G * S;
  OVN_REQUIRE(ctx->head_s == S && G == ctx->head_g && W >= OVN_FEAT_W_MIN && W <= OVN_FEAT_W_MAX, OVN_ERR_STATE,
              "Delta head at width %d: geometry (conv1size %d, %d groups) does not match", W, ctx->head_s, ctx->head_g);
  float *o2 = scratch.o2, *o3 = scratch.o3;
  int rc;
  if (ctx->head_width_split && ctx->head_mode == 1) {   // times its prepare and contraction kernels itself
    rc = ovn_delta_w_split_c12_forward(ctx, feats_l, lidx, feats_r, ridx, n, scratch.scales, o2, stream);
    if (rc) return rc;
  } else {
    OvnProfScope ps(ctx, OVN_K_DELTA, stream);
    const int mt = (G + 15) / 16;
    if (R <= 384)
      rc = mt == 1 ? launch_c12<3, 1>(ctx, feats_l, lidx, feats_r, ridx, n, W, o2, stream)
                   : launch_c12<3, 2>(ctx, feats_l, lidx, feats_r, ridx, n, W, o2, stream);
    else
      rc = mt == 2 ? launch_c12<4, 2>(ctx, feats_l, lidx, feats_r, ridx, n, W, o2, stream)
                   : launch_c12<4, 3>(ctx, feats_l, lidx, feats_r, ridx, n, W, o2, stream);
    if (rc) return rc;
  }
  int oh = 0, ow = 0;
  {
    OvnProfScope ps(ctx, OVN_K_C3, stream);
    rc = ovn_conv_forward(ctx->head.c3, o2, n, G, G, o3, &oh, &ow, stream);    // (n, G, G, 128) -> (n, G - 2, G - 2, 256)
  }
  if (rc) return rc;
  OVN_REQUIRE(oh == G - 2 && ow == G - 2, OVN_ERR_STATE, "Delta head at width %d: c_conv3 produced %dx%d", W, oh, ow);
  OvnProfScope ps(ctx, OVN_K_DENSE, stream);
  return ovn_dense_sigmoid_forward(ctx, o3, n, (long long)(G - 2) * (G - 2) * OVN_C3_OUT, overlap, logit, stream);
}

int ovn_dense_sigmoid_forward(const ovn_ctx* ctx, const float* o3, int n, long long dense_in, float* overlap, float* logit,
                              hipStream_t stream) {
  hipLaunchKernelGGL(dense_sigmoid_kernel, dim3(n), dim3(256), 0, stream, o3, ctx->head.wd, ctx->head.bd, dense_in, overlap, logit);
  OVN_HIP_CHECK(hipGetLastError());
  return OVN_OK;
}
