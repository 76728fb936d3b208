// Delta (overlap) head of OverlapNet at a runtime feature width W (45 <= W <= 512, W != 360) in the split-operand ("f16x3")
// arithmetic of delta_head_f16x3.hip for gfx950: DeltaLayer + c_conv1 + c_conv2 on v_mfma_f32_16x16x32_f16, fp32 accumulate.
// Opt-in (ovn_set_head_width_split); c_conv3 and Dense stay on the fp32 kernels of ovn_delta_forward (delta_head.hip).
//
// Geometry: that of delta_head.hip.  G = W // 15 column groups (3..34), R = 15 G rows of l reach c_conv2, the last W - 15 G
// columns of r are never read.
//
// Arithmetic: as delta_head_f16x3.hip's header defines it.  Every operand x is scaled by a power of two and written hi + lo
// (hi = fp16_rtz(x), lo = fp16_rne(x - hi)); a w = a_hi w_hi + a_lo w_hi + a_hi w_lo, three MFMAs in that order per product, the
// scales divided out of the fp32 accumulators.  Weight fragments and their static scales are the ones the 360 path registers
// (ctx->head.w1p_h, ctx->head.w2p_h, ctx->head.hs): no operand of its own.
//
// The DeltaLayer in ABS FORM: |l - r| is formed in fp32 registers, then split.  The min form of the 360 path buys its cheap inner
// loop (one v_min_u32 per element) with packed copies of both volumes and two linear terms pushed through c_conv2: three more
// kernels whose tiles would all need a run-time G, and a cancellation that costs ~2x in the error bound.  Here the split of
// |l - r| costs 20 VALU instructions per row tile and step (8 v_sub_f32, 4 v_cvt_pkrtz_f16_f32 with |.| as a source modifier, 8
// v_fma_mix{lo,hi}_f16) next to the 12 MFMAs they feed; DESIGN.md section 18 has the measurement and what still limits the kernel.
// The shift c = -min(0, smallest value of the pair) cancels in l - r, so it
// enters only where the 360 path's enters without cancelling: the feature scale is that of the SHIFTED range,
// sa = ovn_pow2_scale_for(max + c), which bounds |l - r| by 2^14 in scaled units whatever the signs.
//
// Scales (delta_w_split_prepare_kernel, per PAIR, from the pair's own two volumes only):
//   sa  = ovn_pow2_scale_for(span), span = max + c over both volumes (all W rows)
//   s1  = ovn_pow2_scale_for(|b1|max + span max_o sum |W1[., o]|): bound of |o1|
//   o1  = acc1 / (sa sw1) + b1;   o2 = relu(acc2 / (s1 sw2) + b2)
//
// One workgroup (8 waves) per pair, for each column group jb:
//   GEMM1  (R x 1920) x (1920 x 64): 60 MFMA steps u = 15 s + dj (channel slice s, tap dj: the K order of ctx->head.w1p_h).  Row tiles
//          go to the waves interleaved, tile = 24 pass + wave + 8 t (t < 3), in ceil(ntiles / 24) passes (1 for R <= 384, else 2);
//          a lane holds its rows of l (scaled, channels 32 g .. 32 g + 31) in registers for the pass, the 15 rows of r sit in LDS
//          (scaled).  The pass is compiled per tile count of a wave (0..3): straight-line steps, no branch around an MFMA.
//          The W1 fragments of a step (8 KB) are shared by all waves through a double-buffered LDS window, one barrier per step.
//   o1     (+ b1, scaled by s1, split) goes to LDS as the hi and lo fp16 A images of GEMM2, [plane][G][968]: row ib, position
//          k' = 64 di + 4 (o & 15) + (o >> 4), the K order of ctx->head.w2p_h.  Rows >= R are computed on zeros and dropped here.
//   GEMM2  (G x 960) x (960 x 128): wave w owns output channels 16 w .. 16 w + 15 for all ceil(G / 16) row tiles; padding rows
//          (>= G) are clamped reads and never stored.
// LDS: 2 G 1936 + 7680 + 16384 bytes: 155,712 at G = 34.  Every output element is summed in one fixed order that depends on W alone.
#include "ovn_internal.h"

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

namespace {

constexpr int FC = OVN_FEAT_C;        // 128
constexpr int S = OVN_S;              // 15
constexpr int O1 = OVN_C1_OUT;        // 64
constexpr int O2 = OVN_C2_OUT;        // 128
constexpr int K2 = S * O1;            // 960
constexpr int NSTEP1 = S * FC / 32;   // 60 MFMA steps of GEMM1
constexpr int NSTEP2 = K2 / 32;       // 30 MFMA steps of GEMM2
constexpr int STEP_BYTES = 8192;      // W1 fragments of one step: [nt(4)][hi/lo][lane(64)][8 fp16]
constexpr int ROWB = 2 * K2 + 16;     // 1936 bytes per o1 image row: an odd number of 16-B slots -> conflict-free b128 row reads
constexpr int RS_BYTES = S * FC * 4;  // 7680
constexpr int G_MAX = OVN_FEAT_W_MAX / S;   // 34
constexpr int TPW = 3;                // row tiles per wave and pass
constexpr int TPP = 8 * TPW;          // row tiles per pass

constexpr size_t lds_bytes(int G) { return (size_t)2 * G * ROWB + RS_BYTES + 2 * STEP_BYTES; }
static_assert(lds_bytes(G_MAX) <= 160 * 1024, "o1 images + r rows + W1 window exceed the LDS of a CU");

// (x0, x1), already scaled -> packed fp16 hi pair (rtz) and lo pair (rne of the exact remainder; `one` = 1.0f in a register keeps
// the fma from being folded into a subtraction that needs two more conversions)
__device__ __forceinline__ void split_pair(float x0, float x1, float one, unsigned& hi_pk, unsigned& lo_pk) {
  const f16x2 h = __builtin_bit_cast(f16x2, __builtin_amdgcn_cvt_pkrtz(x0, x1));
  f16x2 l;
  l[0] = (_Float16)__builtin_fmaf(x0, one, -(float)h[0]);
  l[1] = (_Float16)__builtin_fmaf(x1, one, -(float)h[1]);
  hi_pk = __builtin_bit_cast(unsigned, h);
  lo_pk = __builtin_bit_cast(unsigned, l);
}

__device__ __forceinline__ f32x4 mma(const f16x8& a, const f16x8& b, const f32x4& c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}

// scales[pair] = {sa, 1 / (sa sw1), s1, 1 / (s1 sw2)}.  256 threads, one workgroup per pair; reads all W rows of both volumes.
__global__ __launch_bounds__(256) void delta_w_split_prepare_kernel(const float* __restrict__ feats_l, const int32_t* __restrict__ lidx,
                                                                    const float* __restrict__ feats_r, const int32_t* __restrict__ ridx,
                                                                    int W, float sw1, float sw2, float w1_colsum, float b1_absmax,
                                                                    f32x4* __restrict__ scales) {
  __shared__ float red[8];
  const int pair = blockIdx.x, tid = threadIdx.x;
  const long long fe = (long long)W * FC;
  const f32x4* L = reinterpret_cast<const f32x4*>(feats_l + (long long)(lidx ? lidx[pair] : pair) * fe);
  const f32x4* Rv = reinterpret_cast<const f32x4*>(feats_r + (long long)(ridx ? ridx[pair] : 0) * fe);
  const int nv = W * (FC / 4);
  float mx = -INFINITY, mn = INFINITY;
  for (int i = tid; i < nv; i += 256) {
    const f32x4 a = L[i], b = Rv[i];
    mx = fmaxf(mx, fmaxf(fmaxf(fmaxf(a[0], a[1]), fmaxf(a[2], a[3])), fmaxf(fmaxf(b[0], b[1]), fmaxf(b[2], b[3]))));
    mn = fminf(mn, fminf(fminf(fminf(a[0], a[1]), fminf(a[2], a[3])), fminf(fminf(b[0], b[1]), fminf(b[2], b[3]))));
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    mx = fmaxf(mx, __shfl_down(mx, off, 64));
    mn = fminf(mn, __shfl_down(mn, off, 64));
  }
  if ((tid & 63) == 0) {
    red[tid >> 6] = mx;
    red[4 + (tid >> 6)] = mn;
  }
  __syncthreads();
  if (tid == 0) {
    mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    mn = fminf(fminf(red[4], red[5]), fminf(red[6], red[7]));
    const float c = (mn < 0.0f) ? -mn : 0.0f;   // shift that would make both volumes non-negative: it widens the range to scale
    const float span = mx + c;
    const float sa = ovn_pow2_scale_for(span);
    const float s1 = ovn_pow2_scale_for(b1_absmax + span * w1_colsum);
    scales[pair] = (f32x4){sa, 1.0f / (sa * sw1), s1, 1.0f / (s1 * sw2)};
  }
}

// One pass of GEMM1 + the o1 epilogue for a wave that owns NT (0..3) row tiles tile0, tile0 + 8, ... of it.  NT is a template
// parameter so that the 60 steps are straight-line code; a wave without tiles (NT = 0) still stages W1 and meets the barriers.
template <int NT>
__device__ __forceinline__ void gemm1_pass(const float* __restrict__ L, int R, int tile0,
                                           const u32x4* __restrict__ w1h, const float* __restrict__ b1, const float* rs,
                                           unsigned char* wbuf, unsigned char* img, int planeb, float sa, float inv1, float s1,
                                           float one, int tid, int lane, int lrow, int g) {
  // this lane's rows 16 tile + lrow of l, channels 32 g .. 32 g + 31, scaled.  Loaded per pass and column group (L2 hits, 2 % of a
  // group's time): keeping them across GEMM2 costs more registers than the kernel has.
  f32x4 lreg[NT > 0 ? NT : 1][8];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int i = 16 * (tile0 + 8 * t) + lrow;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      f32x4 v = (i < R) ? *reinterpret_cast<const f32x4*>(L + i * FC + 32 * g + 4 * q) : (f32x4){0.f, 0.f, 0.f, 0.f};
      v[0] *= sa;
      v[1] *= sa;
      v[2] *= sa;
      v[3] *= sa;
      lreg[t][q] = v;
    }
  }
  u32x4 wpend = w1h[STEP_BYTES / 16 + tid];   // step 1
  f32x4 acc[NT > 0 ? NT : 1][4];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) acc[t][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};

#pragma unroll
  for (int s = 0; s < 4; ++s) {
#pragma unroll 1
    for (int dj = 0; dj < S; ++dj) {
      const int u = S * s + dj;
      // W1 of step u + 2 leaves for registers now and is written to the window one iteration later: a load consumed in its own
      // iteration is sunk by the compiler to just before its use, and its whole latency is exposed
      const int un = (u + 2 >= NSTEP1) ? u + 2 - NSTEP1 : u + 2;
      const u32x4 wnew = w1h[un * (STEP_BYTES / 16) + tid];
      if (NT > 0) {
        const unsigned char* wb = wbuf + (u & 1) * STEP_BYTES + 16 * lane;
        const float* rrow = rs + dj * FC + 32 * g + 8 * s;
        const f32x4 r0 = *reinterpret_cast<const f32x4*>(rrow);
        const f32x4 r1 = *reinterpret_cast<const f32x4*>(rrow + 4);
        f16x8 ah[NT > 0 ? NT : 1], al[NT > 0 ? NT : 1];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          const f32x4 l0 = lreg[t][2 * s], l1 = lreg[t][2 * s + 1];
          unsigned h0, h1, h2, h3, q0, q1, q2, q3;
          split_pair(fabsf(l0[0] - r0[0]), fabsf(l0[1] - r0[1]), one, h0, q0);
          split_pair(fabsf(l0[2] - r0[2]), fabsf(l0[3] - r0[3]), one, h1, q1);
          split_pair(fabsf(l1[0] - r1[0]), fabsf(l1[1] - r1[1]), one, h2, q2);
          split_pair(fabsf(l1[2] - r1[2]), fabsf(l1[3] - r1[3]), one, h3, q3);
          ah[t] = __builtin_bit_cast(f16x8, (u32x4){h0, h1, h2, h3});
          al[t] = __builtin_bit_cast(f16x8, (u32x4){q0, q1, q2, q3});
        }
        // per accumulator: a_hi w_hi, then a_lo w_hi, then a_hi w_lo
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
          const f16x8 bh = *reinterpret_cast<const f16x8*>(wb + (2 * nt) * 1024);
          const f16x8 bl = *reinterpret_cast<const f16x8*>(wb + (2 * nt + 1) * 1024);
#pragma unroll
          for (int t = 0; t < NT; ++t) acc[t][nt] = mma(ah[t], bh, acc[t][nt]);
#pragma unroll
          for (int t = 0; t < NT; ++t) acc[t][nt] = mma(al[t], bh, acc[t][nt]);
#pragma unroll
          for (int t = 0; t < NT; ++t) acc[t][nt] = mma(ah[t], bl, acc[t][nt]);
        }
      }
      *reinterpret_cast<u32x4*>(wbuf + ((u + 1) & 1) * STEP_BYTES + 16 * tid) = wpend;   // step u + 1 (step 0 after the last)
      __syncthreads();
      wpend = wnew;
    }
  }

  // o1 = acc / (sa sw1) + b1, scaled by s1 and split -> the A images of GEMM2.  C/D: lane holds column lrow, rows 4g..4g+3 of
  // the tile; its four n-tiles are adjacent in k' (8 bytes per row and plane).  Rows >= R are dropped.
  if (NT > 0) {
    float bv[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) bv[nt] = b1[16 * nt + lrow];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = 16 * (tile0 + 8 * t) + 4 * g + r;
        if (i < R) {
          const int ib = i / S;
          const int di = i - ib * S;
          unsigned h0, h1, q0, q1;
          split_pair((acc[t][0][r] * inv1 + bv[0]) * s1, (acc[t][1][r] * inv1 + bv[1]) * s1, one, h0, q0);
          split_pair((acc[t][2][r] * inv1 + bv[2]) * s1, (acc[t][3][r] * inv1 + bv[3]) * s1, one, h1, q1);
          unsigned char* dst = img + ib * ROWB + (O1 * di + 4 * lrow) * 2;
          *reinterpret_cast<u32x2*>(dst) = (u32x2){h0, h1};
          *reinterpret_cast<u32x2*>(dst + planeb) = (u32x2){q0, q1};
        }
      }
    }
  }
}

template <int MT>
__global__ __launch_bounds__(512) void delta_c12_w_split_kernel(const float* __restrict__ feats_l, const int32_t* __restrict__ lidx,
                                                                const float* __restrict__ feats_r, const int32_t* __restrict__ ridx,
                                                                const u32x4* __restrict__ w1h, const float* __restrict__ b1,
                                                                const u32x4* __restrict__ w2h, const float* __restrict__ b2,
                                                                const f32x4* __restrict__ scales, int W, float one, float* __restrict__ o2) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int G = W / S;
  const int R = G * S;                   // rows of l that reach c_conv2
  const int ntiles = (R + 15) >> 4;
  const int npass = (ntiles + TPP - 1) / TPP;
  unsigned char* img = smem;                                   // [hi/lo][G][ROWB]
  float* rs = reinterpret_cast<float*>(smem + 2 * G * ROWB);   // [15][128], scaled by sa
  unsigned char* wbuf = smem + 2 * G * ROWB + RS_BYTES;        // [2][STEP_BYTES]
  const int planeb = G * ROWB;

  const int pair = blockIdx.x;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // in an SGPR: the tile count below is wave-uniform
  const int lrow = lane & 15;
  const int g = lane >> 4;
  const long long fe = (long long)W * FC;

  const float* L = feats_l + (long long)(lidx ? lidx[pair] : pair) * fe;
  const float* Rv = feats_r + (long long)(ridx ? ridx[pair] : 0) * fe;
  const f32x4 sc = scales[pair];
  const float sa = sc[0], inv1 = sc[1], s1 = sc[2], inv2 = sc[3];
  float* o2p = o2 + (long long)pair * G * G * O2;   // this pair's (G, G, 128) block

  // step 0 of W1 into window 0.  60 steps is even and every pass ends by staging step 0 again, so window (u & 1) holds step u
  // throughout the kernel.
  *reinterpret_cast<u32x4*>(wbuf + 16 * tid) = w1h[tid];

  for (int jb = 0; jb < G; ++jb) {
    __syncthreads();  // the previous group's GEMM2 has finished reading the o1 images; nobody reads rs any more
    if (tid < S * FC / 4) {
      f32x4 v = *reinterpret_cast<const f32x4*>(Rv + jb * S * FC + 4 * tid);
      v[0] *= sa;
      v[1] *= sa;
      v[2] *= sa;
      v[3] *= sa;
      *reinterpret_cast<f32x4*>(rs + 4 * tid) = v;
    }
    __syncthreads();

    for (int pass = 0; pass < npass; ++pass) {
      const int tile0 = TPP * pass + wave;        // this wave's tiles: tile0, tile0 + 8, tile0 + 16, as far as they exist
      int nv = (ntiles - tile0 + 7) >> 3;
      nv = nv < 0 ? 0 : (nv > TPW ? TPW : nv);
      switch (nv) {                               // wave-uniform
        case 3: gemm1_pass<3>(L, R, tile0, w1h, b1, rs, wbuf, img, planeb, sa, inv1, s1, one, tid, lane, lrow, g); break;
        case 2: gemm1_pass<2>(L, R, tile0, w1h, b1, rs, wbuf, img, planeb, sa, inv1, s1, one, tid, lane, lrow, g); break;
        case 1: gemm1_pass<1>(L, R, tile0, w1h, b1, rs, wbuf, img, planeb, sa, inv1, s1, one, tid, lane, lrow, g); break;
        default: gemm1_pass<0>(L, R, tile0, w1h, b1, rs, wbuf, img, planeb, sa, inv1, s1, one, tid, lane, lrow, g); break;
      }
    }
    __syncthreads();

    // GEMM2: wave -> output channels 16 wave .., all MT row tiles
    {
      int arow[MT];   // byte offsets into the hi image
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        int ib = 16 * mt + lrow;
        if (ib > G - 1) ib = G - 1;    // padding rows of the last tile: clamped reads, never stored
        arow[mt] = ib * ROWB + 16 * g;
      }
      const u32x4* wcol = w2h + wave * 128 + lane;
      f32x4 acc2[MT];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) acc2[mt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
      for (int ks = 0; ks < NSTEP2; ++ks) {
        const f16x8 bh = __builtin_bit_cast(f16x8, wcol[ks * 1024]);
        const f16x8 bl = __builtin_bit_cast(f16x8, wcol[ks * 1024 + 64]);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
          const f16x8 ah = *reinterpret_cast<const f16x8*>(img + arow[mt] + 64 * ks);
          const f16x8 al = *reinterpret_cast<const f16x8*>(img + arow[mt] + 64 * ks + planeb);
          acc2[mt] = mma(ah, bh, acc2[mt]);
          acc2[mt] = mma(al, bh, acc2[mt]);
          acc2[mt] = mma(ah, bl, acc2[mt]);
        }
      }
      const int p = 16 * wave + lrow;
      const float bv2 = b2[p];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int ib2 = 16 * mt + 4 * g + r;
          if (ib2 < G) o2p[(ib2 * G + jb) * O2 + p] = fmaxf(acc2[mt][r] * inv2 + bv2, 0.0f);
        }
    }
  }
}

template <int MT>
int launch_split(const ovn_ctx* ctx, const float* feats_l, const int32_t* lidx, const float* feats_r, const int32_t* ridx, int n, int W,
                 const f32x4* scales, float* o2, hipStream_t stream) {
  int rc = ovn_allow_dynamic_lds(reinterpret_cast<const void*>(delta_c12_w_split_kernel<MT>), lds_bytes(G_MAX));
  if (rc) return rc;
  hipLaunchKernelGGL((delta_c12_w_split_kernel<MT>), dim3(n), dim3(512), lds_bytes(W / S), stream, feats_l, lidx, feats_r, ridx,
                     reinterpret_cast<const u32x4*>(ctx->head.w1p_h), ctx->head.b1, reinterpret_cast<const u32x4*>(ctx->head.w2p_h), ctx->head.c2.bias,
                     scales, W, 1.0f, o2);
  OVN_HIP_CHECK(hipGetLastError());
  return OVN_OK;
}

}  // namespace

// Bytes of per-pair scales the split route adds to the scratch of ovn_delta_forward
size_t ovn_delta_w_split_pair_bytes() { return sizeof(f32x4); }

// DeltaLayer + c_conv1 + c_conv2 for n pairs at feature width ctx->feat_w, conv1size 15, in f16x3 arithmetic: o2 (n, G, G, 128).
// `scales`: n * ovn_delta_w_split_pair_bytes() bytes of scratch, 16-byte aligned.
int ovn_delta_w_split_c12_forward(ovn_ctx* ctx, const float* feats_l, const int32_t* lidx, const float* feats_r, const int32_t* ridx,
                                  int n, void* scales, float* o2, hipStream_t stream) {
  const int W = ctx->feat_w, G = W / S;
  OVN_REQUIRE(ctx->head_s == S && G == ctx->head_g && W >= OVN_FEAT_W_MIN && W <= OVN_FEAT_W_MAX && ctx->head.w1p_h && ctx->head.w2p_h,
              OVN_ERR_STATE, "split Delta head at width %d: geometry (conv1size %d, %d groups) or operands do not match", W,
              ctx->head_s, ctx->head_g);
  f32x4* sc = static_cast<f32x4*>(scales);
  {
    OvnProfScope ps(ctx, OVN_K_DELTA_PREP, stream);
    hipLaunchKernelGGL(delta_w_split_prepare_kernel, dim3(n), dim3(256), 0, stream, feats_l, lidx, feats_r, ridx, W, ctx->head.hs.sw1,
                       ctx->head.hs.sw2, ctx->head.hs.w1_colsum, ctx->head.hs.b1_absmax, sc);
    OVN_HIP_CHECK(hipGetLastError());
  }
  OvnProfScope ps(ctx, OVN_K_DELTA, stream);
  const int mt = (G + 15) / 16;
  return mt == 1   ? launch_split<1>(ctx, feats_l, lidx, feats_r, ridx, n, W, sc, o2, stream)
         : mt == 2 ? launch_split<2>(ctx, feats_l, lidx, feats_r, ridx, n, W, sc, o2, stream)
                   : launch_split<3>(ctx, feats_l, lidx, feats_r, ridx, n, W, sc, o2, stream);
}
