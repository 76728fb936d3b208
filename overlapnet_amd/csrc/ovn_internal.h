// Internal declarations shared by the translation units of libovn_hip.so (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/ovn_hip.h"
#include "ovn_scratch.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

// ---- error plumbing -------------------------------------------------------------------------------
void ovn_set_error(const char* fmt, ...);

#define OVN_HIP_CHECK(expr)                                                                   \
  do {                                                                                        \
    hipError_t _e = (expr);                                                                   \
    if (_e != hipSuccess) {                                                                   \
      ovn_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
      return OVN_ERR_HIP;                                                                     \
    }                                                                                         \
  } while (0)

#define OVN_REQUIRE(cond, code, ...)   \
  do {                                 \
    if (!(cond)) {                     \
      ovn_set_error(__VA_ARGS__);      \
      return (code);                   \
    }                                  \
  } while (0)

// Selects a context's device for the duration of a C-ABI call and restores the caller's current device afterwards: a
// process may hold contexts on several GPUs, and a library call must not change which GPU the caller's next allocation
// or kernel lands on.
struct OvnDeviceGuard {
  int prev = -1;
  bool ok = false;
  explicit OvnDeviceGuard(int dev) {
    int cur = -1;
    if (hipGetDevice(&cur) != hipSuccess) return;
    if (cur == dev) {
      ok = true;
      return;
    }
    ok = (hipSetDevice(dev) == hipSuccess);
    if (ok) prev = cur;
  }
  ~OvnDeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
  OvnDeviceGuard(const OvnDeviceGuard&) = delete;
  OvnDeviceGuard& operator=(const OvnDeviceGuard&) = delete;
};
#define OVN_ON_DEVICE(dev)                                                             \
  OvnDeviceGuard ovn_device_guard_(dev);                                               \
  OVN_REQUIRE(ovn_device_guard_.ok, OVN_ERR_HIP, "cannot select HIP device %d", (int)(dev))

// ---- feature geometry fixed by the reference network ----------------------------------------------
constexpr int OVN_FEAT_W = 360;   // leg_output_width, config/network.yml:77
constexpr int OVN_FEAT_C = 128;   // s_conv10 filters, generateNet.py:214
constexpr int OVN_FEAT_ELEMS = OVN_FEAT_W * OVN_FEAT_C;
// the fp32 heads (delta_head.hip, corr_head.hip, delta_head_generic.hip) take the leg output width W at run time, any W in
// [OVN_FEAT_W_MIN, OVN_FEAT_W_MAX] (include/ovn_hip.h); every feature volume is ctx->feat_w * 128 floats.  The constants below that
// derive from 360 describe the shipped configuration, which the split-operand and spectral kernels are tiled around
constexpr int OVN_S = 15;         // conv1NetworkHead_conv1size default, generateNet.py:88-89
constexpr int OVN_G = OVN_FEAT_W / OVN_S;            // 24
constexpr int OVN_C1_OUT = 64;    // c_conv1 filters
constexpr int OVN_C2_OUT = 128;   // c_conv2 filters
constexpr int OVN_C3_OUT = 256;   // c_conv3 filters
constexpr int OVN_O3_HW = OVN_G - 2;                 // 22
constexpr int OVN_DENSE_IN = OVN_O3_HW * OVN_O3_HW * OVN_C3_OUT;  // 123904
constexpr int OVN_A2_IN_YAW_MAX_PAIRS = 64;                  // sweeps up to this many pairs carry the query's A2 tasks in their yaw launch
constexpr int OVN_DENSE_PARTIALS = 12;                        // Dense partial sums per pair left by c3_dense_kernel: 3 row bands x 2 channel halves x 2 m-tile halves
constexpr int OVN_ACTMAX_SLOTS = 32;                           // layers with per-scan activation maxima (f16x3 scales)
constexpr int OVN_LEG_SLICE = 1024;                             // scans per pass of ovn_leg over its ping-pong scratch
constexpr int OVN_ACTMAX_STRIDE = 32;                          // words between the maxima of two scans: every scan's word has its
                                                               // own 128-byte line (atomics on one line serialise at the memory side)
constexpr int OVN_SPEC_W = 368;                                 // floats per spectrum row: Re[0..180] | pad | Im at 184.. | pad
constexpr int OVN_SPEC_ELEMS = OVN_FEAT_C * OVN_SPEC_W;        // 47104 floats = 188,416 B per scan
static_assert(OVN_DELTA_CACHE_ELEMS >= OVN_FEAT_ELEMS + 24 * 128 + 4, "include/ovn_hip.h: OVN_DELTA_CACHE_ELEMS");

// ---- scaled fp16 hi/lo arithmetic ("f16x3") ----------------------------------------------------------
// Power-of-two scale that brings a tensor whose largest magnitude is m into [2^13, 2^14): 2^(14 - e) with 2^(e-1) <= m < 2^e.
// fp16 holds 2^14 with 2x headroom below 65504; m == 0, Inf or NaN -> 1 (nothing to protect).
__host__ __device__ inline float ovn_pow2_scale_for(float m) {
  if (!(m > 0.0f) || !(m < 3.0e38f)) return 1.0f;
  int e = 0;
  (void)frexpf(m, &e);
  int k = 14 - e;
  k = k > 100 ? 100 : (k < -100 ? -100 : k);
  return ldexpf(1.0f, k);
}

#ifdef __HIPCC__
// max |value| of a WORKGROUP folded into one device word: wave shuffle reduction, the waves' maxima through `red` (>= 16 floats of
// LDS that nothing else uses at this point), then at most ONE atomicMax per workgroup (|v| orders like its float bits; skipped when
// it would not raise the word).  Per-wave atomics on per-scan words cost s_conv1 / s_conv2 +75 % (164 k device-scope atomics per
// 1025 scans, all waves of a scan arriving at a zeroed word together).  Every thread of the workgroup must call it.
__device__ __forceinline__ void ovn_fold_absmax_wg(float vmax, unsigned* word, float* red) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) vmax = fmaxf(vmax, __shfl_down(vmax, off, 64));
  const int nw = (blockDim.x + 63) >> 6;
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = vmax;
  __syncthreads();
  if (threadIdx.x == 0) {
    float m = red[0];
    for (int w = 1; w < nw; ++w) m = fmaxf(m, red[w]);
    const unsigned bits = __float_as_uint(m);
    if (m > 0.f && bits > __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(word, bits);
  }
}

// The largest of a workgroup's per-thread values, returned to EVERY thread (a strip or tile that takes its scale from its own
// maximum): wave shuffle reduction, one word of `red` per wave, ONE barrier, every thread reads all NWAVES words.  `red` is NWAVES
// floats of LDS that nothing else uses from the call until a later barrier: whoever writes them next -- a second maximum through
// the same words, or the data `red` was borrowed from -- puts that barrier first.  Every thread of the workgroup must call it.
template <int NWAVES>
__device__ __forceinline__ float ovn_wg_max_all(float m, float* red) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_down(m, off, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  m = red[0];
#pragma unroll
  for (int w = 1; w < NWAVES; ++w) m = fmaxf(m, red[w]);
  return m;
}

// The largest AND the smallest, in the two halves of ovn_wg_max_all for a caller that has LDS work of its own to put in front of the
// barrier: _put = the wave reductions and the waves' words (red[w] maxima, red[NWAVES + w] minima), then the CALLER's barrier, then
// _get on every thread.  `red`: 2 NWAVES floats, under the rule above.
template <int NWAVES>
__device__ __forceinline__ void ovn_wg_minmax_put(float mx, float mn, float* red) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    mx = fmaxf(mx, __shfl_down(mx, off, 64));
    mn = fminf(mn, __shfl_down(mn, off, 64));
  }
  if ((threadIdx.x & 63) == 0) {
    red[threadIdx.x >> 6] = mx;
    red[NWAVES + (threadIdx.x >> 6)] = mn;
  }
}
template <int NWAVES>
__device__ __forceinline__ void ovn_wg_minmax_get(const float* red, float& mx, float& mn) {
  mx = red[0];
  mn = red[NWAVES];
#pragma unroll
  for (int w = 1; w < NWAVES; ++w) {
    mx = fmaxf(mx, red[w]);
    mn = fminf(mn, red[NWAVES + w]);
  }
}

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));

// The leg's scaled hi/lo split: (s d0, s d1) -> hi = fp16_rtz (v_cvt_pkrtz_f16_f32: one instruction per pair), lo = fp16_rne of the
// exact remainder, through v_fma_mixlo/hi_f16 (`one` = 1.0f in a register keeps the compiler from folding the fma into a subtraction
// that needs two more conversions, see delta_head_f16x3.hip).  The Delta head, c3_dense.hip and corr_spectral.hip split under
// arithmetic policies of their own and do not use it.
__device__ __forceinline__ void ovn_split_f16(float d0, float d1, float s, float one, f16x2& hi, f16x2& lo) {
  const float x0 = d0 * s, x1 = d1 * s;
  hi = __builtin_bit_cast(f16x2, __builtin_amdgcn_cvt_pkrtz(x0, x1));
  lo[0] = (_Float16)__builtin_fmaf(x0, one, -(float)hi[0]);
  lo[1] = (_Float16)__builtin_fmaf(x1, one, -(float)hi[1]);
}
__device__ __forceinline__ void ovn_split_f16(f32x4 d, float s, float one, f16x4& hi, f16x4& lo) {
#pragma unroll
  for (int e = 0; e < 4; e += 2) {
    f16x2 h, l;
    ovn_split_f16(d[e], d[e + 1], s, one, h, l);
    hi[e] = h[0];
    hi[e + 1] = h[1];
    lo[e] = l[0];
    lo[e + 1] = l[1];
  }
}
#endif

// ---- normalisation of the correlation head's inputs (NormalizedCorrelation2D normalize=..., ovn_set_corr_normalization) ----------
// Per (volume, channel), over the W columns:
//   1 euclidean        x' = x / sqrt(max(sum x^2, 1e-12))
//   2 scaling          x' = (x - min x) / (max x - min x + 1e-6)
//   3 standardization  y = (x - mean x) + 1e-5, x' = y / sqrt(max(sum y^2, 1e-12))
// all of the form x' = RN32(((x - m) + a) s) with the per-channel m, s and the mode's constant a in fp64; each element is evaluated
// in fp64 and rounded ONCE to fp32.  The statistics are fp64 sums in ONE fixed order: per channel ceil(W / 24) blocks of 24
// consecutive columns (the last one partial unless 24 divides W; 15 whole blocks at W = 360), each summed in column order, then the
// block sums in block order.  Every route (direct head at any width, fused DFT, standalone pass) calls ovn_corr_norm_affine, so a
// volume's normalised values do not depend on the batch, the pair, the launch or the rank.
constexpr int OVN_NORM_BLK = 24;                          // columns per partial sum
constexpr int OVN_NORM_NB = OVN_FEAT_W / OVN_NORM_BLK;    // 15 partial sums per channel at W = 360
static_assert(OVN_NORM_NB * OVN_NORM_BLK == OVN_FEAT_W, "15 whole blocks tile the 360 columns (the spectral kernels' LDS)");
constexpr int OVN_NORM_NB_MAX = (OVN_FEAT_W_MAX + OVN_NORM_BLK - 1) / OVN_NORM_BLK;   // 22 at W = 512

template <int NB, int NCH>
struct OvnNormLds {       // LDS of ovn_corr_norm_affine for up to NB blocks of NCH channels (NB = 15, NCH = 128: 32 KB)
  double part[NB][NCH];
  float mn[NB][NCH], mx[NB][NCH];
  double m[NCH], s[NCH];  // the affine form: x' = RN32(((x - m) + a) s)
};

__host__ __device__ inline double ovn_corr_norm_add(int mode) { return mode == 3 ? 1e-5 : 0.0; }

#ifdef __HIPCC__
__device__ __forceinline__ float ovn_corr_norm_apply(float x, double m, double a, double s) {
  return (float)((((double)x - m) + a) * s);
}

// One block of pass 1 / pass 2 over n consecutive columns of a channel (p: its first element), in column order.  The whole blocks
// pass the constant OVN_NORM_BLK (a constant trip count), the last, partial block its runtime length.
__device__ __forceinline__ void ovn_norm_block_stats(const float* __restrict__ p, int n, double& sm, float& lo, float& hi) {
#pragma unroll 8
  for (int i = 0; i < n; ++i) {
    const float v = p[(size_t)i * OVN_FEAT_C];
    sm += (double)v;
    lo = fminf(lo, v);
    hi = fmaxf(hi, v);
  }
}
__device__ __forceinline__ double ovn_norm_block_sumsq(const float* __restrict__ p, int n, double m, double a) {
  double q = 0.0;
#pragma unroll 8
  for (int i = 0; i < n; ++i) {
    const double y = ((double)p[(size_t)i * OVN_FEAT_C] - m) + a;
    q = __builtin_fma(y, y, q);
  }
  return q;
}

// Affine form of channels c0 .. c0 + NCH - 1 of one (W, 128) feature volume (X = volume + c0, W <= 24 NB) for mode 1..3 into
// L.m / L.s.  Every thread of the (1-D) workgroup must call it; it ends with a barrier, after which L.m / L.s are valid.
template <int NB, int NCH>
__device__ void ovn_corr_norm_affine(const float* __restrict__ X, int W, int mode, OvnNormLds<NB, NCH>& L) {
  const int tid = threadIdx.x, nt = blockDim.x;
  const int nfull = W / OVN_NORM_BLK, tail = W - nfull * OVN_NORM_BLK, nb = nfull + (tail ? 1 : 0);
  for (int t = tid; t < nb * NCH; t += nt) {   // pass 1: block sums, minima, maxima
    const int c = t % NCH, b = t / NCH;
    const float* p = X + (size_t)(b * OVN_NORM_BLK) * OVN_FEAT_C + c;
    double sm = 0.0;
    float lo = INFINITY, hi = -INFINITY;
    if (b < nfull) ovn_norm_block_stats(p, OVN_NORM_BLK, sm, lo, hi);
    else ovn_norm_block_stats(p, tail, sm, lo, hi);
    L.part[b][c] = sm;
    L.mn[b][c] = lo;
    L.mx[b][c] = hi;
  }
  __syncthreads();
  if (tid < NCH) {
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
  for (int t = tid; t < nb * NCH; t += nt) {   // pass 2 (euclidean, standardization): block sums of y^2
    const int c = t % NCH, b = t / NCH;
    const float* p = X + (size_t)(b * OVN_NORM_BLK) * OVN_FEAT_C + c;
    L.part[b][c] = ovn_norm_block_sumsq(p, b < nfull ? OVN_NORM_BLK : tail, L.m[c], a);
  }
  __syncthreads();
  if (tid < NCH) {
    double q = 0.0;
    for (int b = 0; b < nb; ++b) q += L.part[b][tid];
    L.s[tid] = 1.0 / sqrt(q > 1e-12 ? q : 1e-12);
  }
  __syncthreads();
}
#endif

// static scales / norms of the Delta-head weights (delta_head_f16x3.hip)
struct OvnHeadScales {
  float sw1 = 1.f, sw2 = 1.f;     // power-of-two scales of the c_conv1 / c_conv2 kernels
  float sws = 1.f;                // ... of the tap-summed c_conv1 kernel (left-volume linear term)
  float w1_colsum = 0.f;          // max over output channels o of sum |W1[., ., o]|: bound of c_conv1's output per unit input
  float b1_absmax = 0.f;
};

// ---- a convolution layer in MFMA fragment order ----------------------------------------------------
// Raise a kernel's dynamic-LDS limit once per (kernel, device): the attribute is per device, and one process may hold
// contexts on several GPUs.  Thread-safe.
int ovn_allow_dynamic_lds(const void* kernel, size_t bytes);

struct OvnConvLayer {
  std::string name;
  int kh = 0, kw = 0, cin = 0, cout = 0, sh = 1, sw = 1;
  int relu = 1;
  int out_cols = 0;  // 0 = cout; else only the first out_cols output channels are stored, at row stride out_cols
                     // (a layer padded with zero filters so that a wide tile divides cout: the 368-column DFT layers)
  int K = 0;      // kh*kw*cin
  int nkc = 0;    // ceil(K/16)
  float* wp = nullptr;    // [nkc][cout/16][64][4] fragment-ordered copy (device)
  float* bias = nullptr;  // [cout] (device)
  void* wp_h = nullptr;   // optional hi/lo fp16 fragments of sw_h * W, [ceil(K/32)][cout/16][2][64][8] (conv_f16x3.hip)
  float sw_h = 1.f;       // power-of-two weight scale of wp_h
  void* wp_h16 = nullptr; // layers with cin 4 / 16 and kw <= 16: the same fragments in the K order (ky, kx padded to 16, c) of the
                          // pixel-major strip kernel (conv_strip.hip), [kh * 512 / cin... steps][cout/16][2][64][8]
  float* wraw = nullptr;  // leg layers: the kernel as registered, (kh, kw, cin, cout): B operand of the data gradient (leg_backward.hip)
};

// Every device copy the heads keep of the registered head weights, and their static scales: ONE owner.  ovn_set_head_weights builds a
// whole new set beside the one in use and swaps it in only when all of it exists (as ovn_set_leg_layer_weights does for a leg layer);
// release() is the one place that frees a set.
struct OvnHeadWeights {
  float* w1p = nullptr;  // c_conv1 in the K-permuted fragment order of the fused kernel
  float* b1 = nullptr;
  OvnConvLayer c2;       // c_conv2 as a [960][128] GEMM operand in fragment order
  OvnConvLayer c3;       // c_conv3 as a regular conv layer
  void* w1p_h = nullptr;   // c_conv1 / c_conv2 scaled hi/lo fp16 fragments (delta_head_f16x3.hip)
  void* w2p_h = nullptr;
  float* w1raw = nullptr;  // c_conv1 kernel as registered, [1920][64]: B operand of the right-volume linear term
  float* w1sum = nullptr;  // c_conv1 kernel summed over its 15 taps, [128][64]: B operand of the left-volume linear term
  float* w1col = nullptr;  // [64] column sums of the c_conv1 kernel (shift term)
  void* wsp_h = nullptr;   // w1sum as scaled hi/lo fp16 fragments
  float* w2sum = nullptr;  // c_conv2 kernel summed over its 15 taps, [64][128]: the right-volume linear term pushed through c_conv2
  void* w1p_b3 = nullptr;  // c_conv1 / c_conv2 as three bf16 planes in the fragment orders of the f16x3 path (bf16x3 head mode)
  void* w2p_b3 = nullptr;
  float* w2raw = nullptr;  // c_conv2 kernel as registered, [960][128] (k = di * 64 + o): B operand of TT in bf16x3 mode
  float* w3raw = nullptr;  // c_conv3 kernel as registered, [3][3][128][256]: the data gradient of ovn_delta_head_grad
  float* wd = nullptr;     // dense kernel [123904]
  float* bd = nullptr;     // dense bias [1]
  OvnHeadScales hs;
  void release();          // frees every buffer and leaves an empty set (ovn_api.hip)
};

struct ovn_ctx {
  int device = 0;
  int in_h = 0, in_w = 0, in_c = 0;
  std::vector<OvnConvLayer> leg;
  bool finalized = false;
  int feat_w = 0;
  // head
  bool head_set = false;
  int head_s = OVN_S;      // conv1NetworkHead_conv1size (ovn_set_head_geometry); the fast Delta paths serve 15, anything else the
  int head_g = OVN_G;      // general fp32 path of delta_head_generic.hip; head_g = 360 // head_s
  OvnHeadWeights head;     // every device copy of the registered head weights (valid while head_set)
  int leg_mode = 1;        // 0 = fp32 MFMA (conv_f32.hip), 1 = scaled 3-term fp16 split on the fp16 MFMA (conv_f16x3.hip)
  int head_compact = 1;    // ovn_set_head_compaction: 1 = 1-vs-N sweeps drop the query's dead channels from the Delta contraction (exact)
  int proj_trig = 0;       // ovn_set_projection_trig: 0 = NumPy-on-AVX512 (SVML) float32 angles, 1 = correctly rounded float32 angles
  unsigned* actmax = nullptr;   // [layer][scan of the slice][OVN_ACTMAX_STRIDE] float bits of max |layer input| of that scan (f16x3 scales)
  int head_mode = 1;       // 0 = fp32 MFMA (exact fp32), 1 = scaled 3-term fp16 split on the fp16 MFMA (default),
                           // 2 = exact 3-term bf16 split on the bf16 MFMA (operands at least as wide as fp32)
  int head_width_split = 0;  // ovn_set_head_width_split: 1 = head mode 1 runs delta_head_w_f16x3.hip at widths other than 360
  // spectral correlation head: constant twiddle layers (corr_spectral.hip)
  OvnConvLayer dft;        // forward transform as a conv layer (fp32 mode) + its fp16 hi/lo fragments (dft_f16x3_kernel)
  double* tw64 = nullptr;  // [2][360] cos / sin (2 pi m / 360) in fp64: start values of the inverse transform (spectral_corr_kernel)
  int corr_norm = 0;       // ovn_set_corr_normalization: 0 none, 1 euclidean, 2 scaling, 3 standardization
  float* norm_buf = nullptr;   // normalised feature volumes of ovn_spectrum's fp32 transform (modes != 0 with head_mode != 1)
  int64_t norm_buf_n = 0;      // ... volumes it holds
  // optional RCCL communicator of the sharded sweep (comm.hip)
  void* comm = nullptr;
  int comm_rank = 0, comm_world = 1;
  // launch structure of a head call (ovn_set_head_pipeline): pairs per pass over the scratch, pairs per sub-chunk (0 = the whole
  // chunk), streams the sub-chunks alternate between (1 or 2), spectral yaw head on its own side stream
  int64_t head_chunk = 1024;
  int64_t head_sub = 0;
  int head_streams = 1;
  int head_yaw_side = 0;   // measured (profiles/r3a_pipeline_matrix.md): no gain from any of the forked forms, the serial order is the default
  bool aux_ready = false;
  hipStream_t aux[2] = {nullptr, nullptr};
  hipEvent_t ev_fork = nullptr, ev_join[2] = {nullptr, nullptr};
  // scratch
  void* ws = nullptr;
  size_t ws_bytes = 0;
  // where the last ovn_heads call left its c_conv2 / c_conv3 activations (first chunk), for tests
  // optional per-kernel timing with HIP events on the launch stream (ovn_profile_begin/end)
  bool prof = false;
  struct ProfRec {
    hipEvent_t a, b;
    int kind;
  };
  std::vector<ProfRec> prof_recs;
  const float* dbg_o2 = nullptr;
  const float* dbg_o3 = nullptr;   // fp32 head mode only; in f16x3 mode o3 is recomputed on request (dbg_partial = scratch)
  float* dbg_partial = nullptr;
  const unsigned* dbg_o2max = nullptr;
  int64_t dbg_n = 0;
  unsigned* c3_arrived = nullptr;       // arrival counters of c3_dense_kernel, one per pair of a chunk, zero between launches
  int64_t c3_arrived_n = 0;
  const unsigned* dbg_live = nullptr;   // live-channel list of the most recent Delta sweep (NULL: it walked all 128 channels; reset
                                        // by every head call and with the scratch it points into)
  // segmented batches (ovn_heads_segments / ovn_top_k_segments): the host segment table staged in pinned memory and copied to
  // seg_dev, both laid out by SegTable (ovn_api.hip: offsets | query_idx | per-pair right index | segment index); seg_ev orders the reuse of seg_host
  void* seg_host = nullptr;
  void* seg_dev = nullptr;
  size_t seg_cap = 0;
  hipEvent_t seg_ev = nullptr;        // the table left seg_host
  hipEvent_t seg_done = nullptr;      // the kernels of the last segmented call have read seg_dev
  bool seg_ev_pending = false;
};

// kernel classes reported by ovn_profile_end
enum { OVN_K_LEG = 0, OVN_K_CORR = 1, OVN_K_DELTA = 2, OVN_K_C3 = 3, OVN_K_DENSE = 4, OVN_K_PROJ = 5, OVN_K_SPECTRUM = 6,
       OVN_K_CORR_SPECTRAL = 7, OVN_K_DELTA_PREP = 8, OVN_K_DELTA_C2 = 9, OVN_K_COUNT = 10 };

struct OvnProfScope {
  ovn_ctx* ctx;
  hipStream_t stream;
  hipEvent_t a = nullptr, b = nullptr;
  int kind;
  OvnProfScope(ovn_ctx* c, int k, hipStream_t s) : ctx(c), stream(s), kind(k) {
    if (ctx->prof && hipEventCreate(&a) == hipSuccess && hipEventCreate(&b) == hipSuccess) (void)hipEventRecord(a, stream);
  }
  ~OvnProfScope() {
    if (ctx->prof && a && b) {
      (void)hipEventRecord(b, stream);
      ctx->prof_recs.push_back({a, b, kind});
    }
  }
};

int ovn_ws_reserve(ovn_ctx* ctx, size_t bytes, hipStream_t stream);
// The scratch is about to be overwritten (or has moved): the debug hooks of an earlier head call pointed into it.  The ONE place that
// clears them; ovn_ws_reserve calls it when the block moves, every call that reuses the block for something else calls it itself.
void scratch_overwritten(ovn_ctx* ctx);
// The scratch of a call, laid out by L (ovn_scratch.h) for the shape `a...`: measure, reserve exactly that, THEN place -- the reserve
// may move the block, so nothing is carved before it.
template <class L, class... A>
int ovn_ws_layout(ovn_ctx* ctx, hipStream_t stream, L* out, const A&... a) {
  int rc = ovn_ws_reserve(ctx, ovn_scratch_bytes<L>(a...), stream);
  if (rc) return rc;
  OvnCarver c(ctx->ws);
  *out = L(c, a...);
  return OVN_OK;
}

// ---- kernels' host launchers (each returns an OVN_* code) ------------------------------------------
// conv_f32.hip
int ovn_conv_prepare(OvnConvLayer* L, const float* kernel_dev, const float* bias_dev, hipStream_t stream);
void ovn_conv_release(OvnConvLayer* L);
int ovn_conv_forward(const OvnConvLayer& L, const float* in, int nb, int h, int w, float* out, int* oh,
                     int* ow, hipStream_t stream);

// conv_f16x3.hip
// scaled fp16 hi/lo fragments of the layer (wp_h, sw_h); synchronises `stream` (the weight maximum is read back)
int ovn_conv_prepare_f16x3(OvnConvLayer* L, const float* kernel_dev, hipStream_t stream);
// in_max[scan]: float bits of max |in| of every scan of the call (device words, left there by the producer of `in` or by
// ovn_absmax_forward); out_max: NULL, or zeroed device words [scan] into which max |out| of every scan is folded for the next
// layer.  Scales are per SCAN and every call size takes the same kernels: a scan's result does not depend on its batch.
int ovn_conv_forward_f16x3(const OvnConvLayer& L, const float* in, int nb, int h, int w, float* out, int* oh, int* ow,
                           const unsigned* in_max, unsigned* out_max, hipStream_t stream);
int ovn_absmax_forward(const float* x, int n_scans, long long per_scan, unsigned* out_max, hipStream_t stream);

// delta_head.hip: the fp32 Delta head at the context's feature width with conv1size 15 (fused fp32 MFMA DeltaLayer + c_conv1 +
// c_conv2, generic c_conv3, Dense); scratch: an OvnDeltaF32Scratch for at least n pairs
int ovn_delta_prepare_w1(OvnHeadWeights* hw, const float* c1_kernel_dev, hipStream_t stream);   // fills hw->w1p
struct OvnDeltaF32Scratch {   // o2 (n, G, G, 128) | o3 (n, G - 2, G - 2, 256) | the split route's per-pair scales (`split` only)
  float *o2 = nullptr, *o3 = nullptr;
  void* scales = nullptr;
  OvnDeltaF32Scratch() = default;
  OvnDeltaF32Scratch(OvnCarver& c, int64_t n, int G, bool split);
};
size_t ovn_delta_pair_bytes(int G);   // what a pair costs, unaligned: the chunk size of a head call derives from it
int ovn_delta_forward(ovn_ctx* ctx, const float* feats_l, const int32_t* lidx, const float* feats_r, const int32_t* ridx, int n,
                      const OvnDeltaF32Scratch& scratch, float* overlap, float* logit, hipStream_t stream);
// Dense(1) + sigmoid over dense_in floats per pair (fixed reduction order)
int ovn_dense_sigmoid_forward(const ovn_ctx* ctx, const float* o3, int n, long long dense_in, float* overlap, float* logit,
                              hipStream_t stream);

// delta_head_f16x3.hip.  An OvnDeltaSubScratch (caller-owned: 2.9 MB per pair) holds the per-pair scales, both packed volumes, the
// linear terms and the c_conv1 min-term rows between the two kernels of a call on n pairs (one sub-chunk); its o2max, the per-pair
// maxima of the c_conv2 output, is the input of ovn_c3_dense_forward.  The f16x3 and bf16x3 paths share it.
int ovn_delta_prepare_f16x3(OvnHeadWeights* hw, const float* c1_kernel_dev, const float* c1_bias_dev, const float* c2_kernel_dev,
                            hipStream_t stream);
struct OvnDeltaSubScratch {
  f32x4* scales = nullptr;
  unsigned *o2max = nullptr, *pl = nullptr, *pr = nullptr;
  float *lin = nullptr, *a2raw = nullptr, *o1raw = nullptr;   // a2raw: one right volume, or n with per_pair_right (unused by a segmented pass)
  void* desc = nullptr;                                       // n DeltaDesc
  unsigned *qblock = nullptr, *live = nullptr;
  _Float16* w1c = nullptr;
  OvnDeltaSubScratch() = default;
  OvnDeltaSubScratch(OvnCarver& c, int n, bool per_pair_right);
};
struct OvnDeltaSegScratch {   // per-segment query state of a segmented pass: A2raw, query block, live list, gathered W1 fragments
  float* a2raw = nullptr;
  unsigned *qblock = nullptr, *live = nullptr;
  _Float16* w1c = nullptr;
  OvnDeltaSegScratch() = default;
  OvnDeltaSegScratch(OvnCarver& c, int nseg);
};
size_t ovn_delta_f16x3_scratch_bytes(int n, bool per_pair_right);   // = the size of an OvnDeltaSubScratch: a sub-chunk's block
// A pass of ovn_heads_segments over the pairs of segments seg0 .. seg0 + nseg - 1 (f16x3, compaction on): pseg = the pass's first
// pair's entry of the per-pair segment index, qidx / offs = the whole batch's query indices and offsets (device), state = the
// per-segment query state, laid out for nseg segments.  ridx must hold each pair's query index.
struct OvnSegPass {
  const int32_t* pseg;
  const int32_t* qidx;
  const int64_t* offs;
  int seg0, nseg;
  OvnDeltaSegScratch state;
};
size_t ovn_delta_f16x3_seg_bytes(int nseg);   // = the size of an OvnDeltaSegScratch
int ovn_delta_c12_f16x3_forward(ovn_ctx* ctx, const float* feats_l, const int32_t* lidx, const float* feats_r,
                                const int32_t* ridx, int n, const OvnDeltaSubScratch& scratch, float* o2, hipStream_t stream,
                                int pair0 = 0,    // pair0: index of the call's first pair in the sweep (rotation of the K walks)
                                const float* dcache_l = nullptr,   // Delta cache rows of the left pool (ovn_delta_cache), 1-vs-N only
                                bool a2_done = false,    // A2raw of the (single) right volume is already in scratch.a2raw
                                const struct OvnSegPass* seg = nullptr);   // a segmented pass (ovn_heads_segments), see above
// bf16x3 head mode: the same two-kernel path with the exact bf16 split (delta_head_f16x3.hip) on the same scratch layout
int ovn_delta_c12_bf16x3_forward(ovn_ctx* ctx, const float* feats_l, const int32_t* lidx, const float* feats_r, const int32_t* ridx,
                                 int n, const OvnDeltaSubScratch& scratch, float* o2, hipStream_t stream, int pair0, bool a2_done);
int ovn_delta_cache_forward(ovn_ctx* ctx, const float* feats, int n, float* cache, hipStream_t stream);
int ovn_delta_walk_stats(ovn_ctx* ctx, int32_t* out16, hipStream_t stream);

// delta_head_generic.hip: the Delta head for any conv1size (fp32, generality path) at feature width ctx->feat_w
struct OvnDeltaGenericScratch {   // out1 (n, W, G, 64) | o2 (n, G, G, 128) | o3 (n, G - 2, G - 2, 256)
  float *out1 = nullptr, *o2 = nullptr, *o3 = nullptr;
  OvnDeltaGenericScratch() = default;
  OvnDeltaGenericScratch(OvnCarver& c, int64_t n, int W, int G);
};
size_t ovn_delta_generic_pair_bytes(int W, int G);   // the layout of ONE pair: the chunk sizes of the fp32 and training calls derive from it
int ovn_delta_generic_forward(const ovn_ctx* ctx, const float* feats_l, const int32_t* lidx, const float* feats_r,
                              const int32_t* ridx, int n, const OvnDeltaGenericScratch& scratch, float* overlap, float* logit,
                              hipStream_t stream);
int ovn_delta_generic_c1_wide(const ovn_ctx* ctx, int FW, const float* feats_l, const int32_t* lidx, const float* feats_r,
                              const int32_t* ridx, int n, float* out1, hipStream_t stream);

// delta_head_backward.hip: weight gradients of the Delta head (ovn_delta_head_grad) at feature width FW; sizes8 as ovn_head_param_sizes
void ovn_head_param_sizes_of(int s, int FW, int64_t* sizes8);
int ovn_delta_head_grad_run(ovn_ctx* ctx, int FW, const float* feats_l, const int32_t* lidx, const float* feats_r, const int32_t* ridx,
                            int64_t n, const float* target, int loss, float scale, float* grad, float* loss_out, float* overlap,
                            float* o2_out, float* o3_out, hipStream_t stream,
                            float* dfeat_l = nullptr, float* dfeat_r = nullptr,   // ovn_heads_feature_grad: per-pair (n, FW, 128) rows, zeroed by the caller
                            bool forward_only = false);                           // overlap (and o2 / o3) alone; grad may then be NULL, as with dfeat_l

// heads_feature_grad.hip: the data gradients behind ovn_heads_feature_grad.  ovn_delta_data_grad: the overlap part of a chunk of np
// pairs from its dO1 (np, FW, G, 64), stored to rows < R of dfeat_l / dfeat_r (np, FW, 128).  ovn_yaw_grad_run: correlation logits
// (to `corr` if given), yaw loss (loss_yaw, 1 float) and its gradient ADDED to dfeat_l / dfeat_r; yaw_bin NULL: the logits alone
int ovn_delta_data_grad(ovn_ctx* ctx, int FW, const float* feats_l, const int32_t* lidx, const float* feats_r, const int32_t* ridx,
                        const float* dO1, int np, float* dfeat_l, float* dfeat_r, hipStream_t stream);
int ovn_yaw_grad_run(ovn_ctx* ctx, int FW, const float* feats_l, const int32_t* lidx, const float* feats_r, const int32_t* ridx,
                     int64_t n, const float* target, const int32_t* yaw_bin, float yaw_scale, float thr, float* dfeat_l, float* dfeat_r,
                     float* loss_yaw, float* corr, hipStream_t stream);

// leg_backward.hip: one leg layer's gradients (ovn_leg_backward, ovn_debug_conv_grad).  dym (nb, oh, ow, cout): dL/d(output) already
// multiplied by [output > 0].  acc_kernel / acc_bias: fp64 running sums in the Keras layouts, onto which the layer's partials are
// added in (scan block, piece) order; part: ovn_leg_grad_part_bytes(L, h, w, nb) bytes of scratch; dx (nb, h, w, cin) is stored times
// [mask > 0] when mask is given; dx, acc_kernel and acc_bias may each be NULL
size_t ovn_leg_grad_part_bytes(const OvnConvLayer& L, int h, int w, int nb);
int ovn_leg_mask_forward(const float* dy, const float* y, float* out, long long n, hipStream_t stream);
int ovn_leg_grad_round(const double* acc, float* out, long long n, hipStream_t stream);
int ovn_leg_layer_backward(const OvnConvLayer& L, const float* x, const float* dym, int nb, int h, int w, float* dx, const float* mask,
                           double* acc_kernel, double* acc_bias, double* part, hipStream_t stream);

// delta_head_w_f16x3.hip: DeltaLayer + c_conv1 + c_conv2 of ovn_delta_forward in f16x3 arithmetic at widths other than 360 (ovn_set_head_width_split with head
// mode 1): o2 (n, G, G, 128) from n * ovn_delta_w_split_pair_bytes() bytes of per-pair scales (OvnDeltaF32Scratch::scales)
size_t ovn_delta_w_split_pair_bytes();
int ovn_delta_w_split_c12_forward(ovn_ctx* ctx, const float* feats_l, const int32_t* lidx, const float* feats_r, const int32_t* ridx,
                                  int n, void* scales, float* o2, hipStream_t stream);

// corr_head.hip: the direct correlation head at feature width W (fp32 MFMA)
// norm_mode: ovn_set_corr_normalization (0 = none; else both volumes normalised on load)
int ovn_corr_forward(const float* feats_l, const int32_t* lidx, const float* feats_r, const int32_t* ridx, int n, int W,
                     int32_t* yaw, float* corr, hipStream_t stream, int norm_mode);

// corr_spectral.hip
int ovn_spectral_prepare(ovn_ctx* ctx, hipStream_t stream);
int ovn_spectrum_forward(ovn_ctx* ctx, const float* feats, int n, float* spectra, hipStream_t stream);
// conv_strip.hip: LDS-resident strip kernels for the leg layer shapes of its table (f16x3 mode); the three look a layer up in that
// one table, so `matches` and a 16-byte aligned input imply that `try` launches
bool ovn_conv_strip_own_scale(const OvnConvLayer& L, int h, int w);
bool ovn_conv_strip_matches(const OvnConvLayer& L, int h, int w);
int ovn_conv_strip_try(const OvnConvLayer& L, const float* in, int nb, int h, int w, float* out, const unsigned* in_max,
                       unsigned* out_max, hipStream_t stream);

// leg_front.hip: s_conv1 + s_conv2 of the C = 4 network fused (f16x3): the 850 KB activation between them stays in LDS
bool ovn_leg_front_matches(const ovn_ctx* ctx, size_t first, int h, int w);
int ovn_leg_front_forward(const ovn_ctx* ctx, size_t first, const float* in, int nb, int h, int w, float* out, int* oh_out, int* ow_out,
                          unsigned* out_max, hipStream_t stream);

// leg_tail.hip: the last six leg layers (1 x {9,9,9,7,5,3}, 128 -> 128) fused, activations carried through LDS (f16x3, batched calls)
bool ovn_leg_tail_matches(const ovn_ctx* ctx, size_t first, int h, int w);
int ovn_leg_tail_forward(const ovn_ctx* ctx, size_t first, const float* in, int nb, int w, float* out, hipStream_t stream);

// c3_dense.hip: c_conv3 + Flatten + Dense fused (f16x3 mode), input patch resident in LDS
// o2max: the per-pair maxima of o2 left by the f16x3 Delta kernel (scale of the fp16 split)
int ovn_c3_dense_forward(const ovn_ctx* ctx, const float* o2, const unsigned* o2max, int n, float* partial, float* o3,
                         unsigned* arrived, float* overlap, float* logit, hipStream_t stream);

// overlap_gt.hip
int ovn_gt_range_forward(const float* points, const int64_t* offsets, int n_scans, long long max_points, const double* ref_poses,
                         const double* inv_cur_pose, int H, int W, double fov_up_deg, double fov_down_deg, double max_range,
                         float* range_out, hipStream_t stream);
int ovn_gt_count_forward(const float* ref_ranges, const float* cur_range, int n, int npix, int32_t* counts, hipStream_t stream);
// counts[f * n_refs + r] of frame frame_idx[f] against scan ref_idx[r] from two LDS bit planes, one workgroup per pair
int ovn_gt_pair_forward(const float* points, const int64_t* offsets, int n_scans, const double* poses, const double* inv_poses,
                        const float* cur_ranges, const int32_t* frame_idx, int n_frames, const int32_t* ref_idx, int n_refs, int H,
                        int W, double fov_up_deg, double fov_down_deg, double max_range, int frame_fastest, int32_t* counts,
                        hipStream_t stream);
int ovn_best_match_forward(const float* overlap, const int32_t* yaw, const int32_t* ids, int n, float threshold,
                           int index_offset, int32_t* out, hipStream_t stream);
// top_k.hip
int ovn_top_k_forward(const float* overlap, const int32_t* yaw, const int32_t* ids, int n, int k, float threshold,
                      int index_offset, int32_t* out, hipStream_t stream);
// one workgroup per segment b: ovn_top_k_forward on overlap[offs[b] .. offs[b + 1]) (yaw / ids sliced alike) -> out + 4 k b
int ovn_top_k_segments_forward(const float* overlap, const int32_t* yaw, const int32_t* ids, const int64_t* offs_dev, int B, int k,
                               float threshold, int32_t* out, hipStream_t stream);
// ridx[p] = qidx[b] and pseg[p] = b (pseg may be NULL) for offs[b] <= p < offs[b + 1]: the per-pair query and segment of a batch
int ovn_segment_ridx_forward(const int64_t* offs_dev, const int32_t* qidx_dev, int B, int n, int32_t* ridx, int32_t* pseg,
                             hipStream_t stream);
// icp_register.hip: one workgroup per pair, all passes in one launch
int ovn_icp_register_forward(const float* vertex, const float* normal, const float* range, int n_scans, int H, int W,
                             double fov_up_deg, double fov_down_deg, double max_range, const int32_t* src_idx, const int32_t* tgt_idx,
                             int n_pairs, const double* init_pose, int iterations, double max_dist, double cos_min, double huber,
                             int min_inliers, double* pose, double* stats, double* system, hipStream_t stream);
// mcl.hip: the particle filter of the overlap-based localization (ovn_mcl_*); motion6 = dx, dy, dtheta, sigma_x, sigma_y, sigma_theta
int ovn_mcl_predict_forward(float* particles, int P, const double* motion6, uint64_t seed, uint64_t step, const int32_t* cell_frame,
                            double origin_x, double origin_y, double resolution, int nx, int ny, int M, int32_t* particle_frame,
                            int32_t* frame_slot, int32_t* frame_list, int32_t* record, hipStream_t stream);
int ovn_mcl_update_forward(float* particles, int P, const int32_t* particle_frame, const int32_t* frame_slot, const float* frame_yaw,
                           int M, const float* overlap, const int32_t* yaw, int U, double sigma_yaw, double eps_yaw, double overlap_min,
                           double* estimate, double* spread, hipStream_t stream);
int ovn_mcl_resample_forward(const float* particles, int P, uint64_t seed, uint64_t step, float* out, int n_out, int32_t* ancestor,
                             int32_t* record, hipStream_t stream);
// a2_feats_r / a2raw non-NULL (small 1-vs-N sweeps): the launch also computes A2raw of that right volume (delta_a2.h) in extra workgroups
int ovn_corr_spectral_forward(ovn_ctx* ctx, const float* spec_l, const int32_t* lidx, const float* spec_r,
                              const int32_t* ridx, int n, int32_t* yaw, float* corr, hipStream_t stream,
                              const float* a2_feats_r = nullptr, float* a2raw = nullptr);

// projection.hip
int ovn_project_forward(ovn_ctx* ctx, const float* points, const int64_t* offsets, int n_scans,
                        int64_t max_points, int H, int W, double fov_up_deg, double fov_down_deg,
                        double max_range, float* range, float* vertex, float* intensity, int32_t* idx,
                        float* normal, float* stacked, int use_depth, int use_normals, int use_intensity,
                        hipStream_t stream);

int ovn_project_semantic_forward(ovn_ctx* ctx, const float* points, const int64_t* offsets, int n_scans, int64_t max_points, int H,
                                 int W, double fov_up_deg, double fov_down_deg, double max_range, const float* probs, int n_classes,
                                 float* range, float* vertex, float* intensity, int32_t* idx, float* normal, float* semantic,
                                 int32_t* sem_idx, float* stacked, int use_depth, int use_normals, int use_semantic, int use_intensity,
                                 hipStream_t stream);
int ovn_projection_angles_forward(const float* points, int64_t n, int H, int W, double fov_up_deg, double fov_down_deg,
                                  double max_range, float* yaw, float* pitch, int32_t* pixel, hipStream_t stream, int trig = 0);
int ovn_normals_forward(const float* range, const float* vertex, int n_scans, int H, int W, float* normal,
                        hipStream_t stream);
int ovn_normals_stack_forward(const float* range, const float* vertex, int n_scans, int H, int W, float* normal, float* stacked,
                              int use_depth, int use_normals, hipStream_t stream);

// A rolling window over the fixed lattice p = origin + (float)(I, J, K) voxel (ovn_tsdf_window_*): the storage
// (nz,ny,nx) holds the samples base <= (I, J, K) < base + n, sample I in slot I mod n (floor modulus) on every axis.  slot0 = the slot of
// `base`; n, base and so slot0 are multiples of 8.  The TSDF kernels are templated on this addressing: a NULL ring is the dense volume.
struct OvnRing {
  int base[3];
  int slot0[3];
};
// the slot of lattice index I on an axis of n slots: a compare and a subtract, no division (base <= I < base + n)
__host__ __device__ __forceinline__ int ovn_ring_slot(int I, int base, int slot0, int n) {
  const int s = slot0 + (I - base);
  return s >= n ? s - n : s;
}
// the lattice index that lives in slot s
__host__ __device__ __forceinline__ int ovn_ring_index(int s, int base, int slot0, int n) {
  return base + (s - slot0) + (s < slot0 ? n : 0);
}

// tsdf.hip: the arguments are those of ovn_tsdf_integrate / ovn_tsdf_triangles, validated there (n_scans >= 1).  With a ring they are
// those of ovn_tsdf_window_integrate / ovn_tsdf_window_triangles: origin is the anchor, box_lo / box_hi the cells to extract
int ovn_tsdf_integrate_forward(ovn_ctx* ctx, float* tsdf, float* weight, int nx, int ny, int nz, const double* origin, double voxel,
                               double trunc, double max_weight, const float* range, const double* poses, int n_scans, int H, int W,
                               double fov_up_deg, double fov_down_deg, double max_range, hipStream_t stream,
                               const OvnRing* ring = nullptr);
int ovn_tsdf_triangles_forward(ovn_ctx* ctx, const float* tsdf, const float* weight, int nx, int ny, int nz, const double* origin,
                               double voxel, double min_weight, float* triangles, int64_t capacity, int64_t* n_triangles,
                               hipStream_t stream, const OvnRing* ring = nullptr, const int* box_lo = nullptr,
                               const int* box_hi = nullptr);
// tsdf_window.hip: the arguments are those of ovn_tsdf_window_shift, validated there
int ovn_tsdf_window_shift_forward(float* tsdf, float* weight, int nx, int ny, int nz, const int* old_base, const int* new_base,
                                  hipStream_t stream);

// tsdf_raycast.hip: the arguments are those of ovn_tsdf_raycast / ovn_tsdf_bricks, validated there (n >= 1; K = the sample count of
// ovn_tsdf_raycast_samples, which counts k with min_range + (float)k step < max_range in f32 up to cap + 1)
long long ovn_tsdf_raycast_samples(double min_range, double max_range, double step, long long cap);
int ovn_tsdf_raycast_forward(ovn_ctx* ctx, const float* tsdf, const float* weight, int nx, int ny, int nz, const double* origin,
                             double voxel, double min_weight, const uint8_t* bricks, const double* poses, int64_t n, int H, int W,
                             const float* cos_az, const float* sin_az, const float* cos_pitch, const float* sin_pitch, double min_range,
                             double step, int K, float* range, float* vertex, float* normal, float* stacked, int use_depth,
                             int use_normals, hipStream_t stream, const OvnRing* ring = nullptr);
int ovn_tsdf_bricks_forward(const float* weight, int nx, int ny, int nz, double min_weight, uint8_t* bricks, hipStream_t stream);

// render_mesh.hip: nodes / order NULL = every ray walks all T triangles; the arguments are those of ovn_render_scans, validated there
int ovn_render_scans_forward(ovn_ctx* ctx, const float* vertices, int V, const int32_t* triangles, int T, const float* nodes,
                             const int32_t* order, int NL, const double* poses, int64_t n, int H, int W, const float* cos_az,
                             const float* sin_az, const float* cos_pitch, const float* sin_pitch, double max_range, float* range,
                             int32_t* tri_id, float* vertex, float* normal, float* stacked, int use_depth, int use_normals,
                             hipStream_t stream);

// selftest.hip
int ovn_mfma_selftest(hipStream_t stream);
