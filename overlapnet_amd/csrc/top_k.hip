// Top-k loop-closure candidates of a 1-vs-N sweep on gfx950: the k best scores leave the GPU as k 16-byte records, best first.
//
// The order is best_match.hip's, extended to a ranked list: overlap descending, equal overlaps by position ascending (np.argmax
// over the reference list picks the first maximum), -0 == +0, NaN never selected.  Every element gets a unique 64-bit key
//     key = ordered(overlap) << 32 | ~position
// (ordered(): the float bits mapped to an unsigned integer that sorts like the float, -0 canonicalised to +0 first), so the k
// largest keys are exactly the wanted records in the wanted order and no step depends on thread scheduling.
//
// One 1024-thread workgroup, one launch, no scratch (like best_match_kernel: N is a few 1e5 scores):
//   1. radix select of the k-th largest key, 8-bit digits from the top: one pass over the scores per digit, a 256-bin LDS
//      histogram of the keys that agree with the digits chosen so far.  The histogram is kept as 32 copies, copy = lane % 32,
//      laid out bin-major, so the 32 lanes of a half-wave always add to 32 different banks -- overlaps crowd into one or two
//      exponent bins, and a single histogram would serialise those adds.  The select stops as soon as the chosen bin holds
//      exactly the keys still needed; position digits that are the same for every position < n are skipped without a pass;
//   2. the keys >= the pivot (exactly min(k, #non-NaN) of them) are appended to an LDS array in any order -- the keys are unique;
//   3. a bitonic sort in LDS puts them best first, and thread i writes record i with ONE 16-byte store.
#include "ovn_internal.h"

namespace {

constexpr int TK_THREADS = 1024;
constexpr int TK_BINS = 256;
constexpr int TK_COPIES = 32;               // histogram copies: one per LDS bank of a half-wave's ds_add_u32

typedef int i32x4 __attribute__((ext_vector_type(4)));

// The high word of a key: the float bits mapped to an unsigned integer that sorts like the float, or 0 for NaN (a valid high word is
// never 0: it is at least ordered(-inf) = 0x007fffff).  The low word is ~position.
__device__ __forceinline__ uint32_t ordered(uint32_t bits) {
  const uint32_t mag = bits & 0x7fffffffu;
  if (mag > 0x7f800000u) return 0;                                  // NaN
  if (mag == 0) bits = 0;                                           // -0 == +0 (on the bits: no dependence on the denormal mode)
  return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
}

// f(position, float bits) over overlap[0, n).  When the array is 16-byte aligned (the usual torch allocation): 16-byte loads, TK_UNROLL
// of them issued before any is used -- one workgroup streams the scores, so loads in flight per thread set the pass time.
constexpr int TK_UNROLL = 8;
template <typename F>
__device__ __forceinline__ void for_each_score(const float* __restrict__ overlap, int n, F f) {
  const uint32_t* p = reinterpret_cast<const uint32_t*>(overlap);
  int tail = 0;
  if ((reinterpret_cast<uintptr_t>(overlap) & 15) == 0) {
    const int n4 = n >> 2;
    const i32x4* p4 = reinterpret_cast<const i32x4*>(overlap);
    for (int base = threadIdx.x; base < n4; base += TK_UNROLL * TK_THREADS) {
      i32x4 v[TK_UNROLL];
#pragma unroll
      for (int u = 0; u < TK_UNROLL; ++u) {
        const int i = base + u * TK_THREADS;
        v[u] = i < n4 ? p4[i] : (i32x4){0, 0, 0, 0};
      }
#pragma unroll
      for (int u = 0; u < TK_UNROLL; ++u) {
        const int i = base + u * TK_THREADS;
        if (i < n4) {
          f(4 * i + 0, (uint32_t)v[u].x);
          f(4 * i + 1, (uint32_t)v[u].y);
          f(4 * i + 2, (uint32_t)v[u].z);
          f(4 * i + 3, (uint32_t)v[u].w);
        }
      }
    }
    tail = n4 << 2;
  }
  // unsigned: tail + threadIdx.x and the last i + TK_THREADS pass 2^31 - 1 when n is within TK_THREADS of it (n < 2^31 always)
  for (uint32_t i = (uint32_t)tail + threadIdx.x; i < (uint32_t)n; i += TK_THREADS) f((int)i, p[i]);
}

// SEG = false: ovn_top_k, one workgroup on overlap[0, n).  SEG = true: ovn_top_k_segments, workgroup b on segment b =
// [offs[b], offs[b + 1]) of overlap / yaw / ids (positions and records relative to the segment), records to out + 4 k b; n and
// index_offset are ignored.  The rest of the kernel is the same code: a segment gets the records of ovn_top_k on its slice.
template <bool SEG>
__global__ __launch_bounds__(TK_THREADS) void top_k_kernel(const float* __restrict__ overlap, const int32_t* __restrict__ yaw,
                                                           const int32_t* __restrict__ ids, int n, int k, float threshold,
                                                           int index_offset, int32_t* __restrict__ out,
                                                           const int64_t* __restrict__ offs) {
  if constexpr (SEG) {
    const int64_t b = blockIdx.x;
    const int64_t base = offs[b];
    n = (int)(offs[b + 1] - base);
    overlap += base;
    if (yaw) yaw += base;
    if (ids) ids += base;
    out += (size_t)b * k * 4;
    index_offset = 0;
  }
  __shared__ uint32_t hist[TK_BINS * TK_COPIES];     // 32 KB: hist[bin * 32 + copy]
  __shared__ uint32_t merged[TK_BINS];
  __shared__ uint64_t keys[OVN_TOP_K_MAX];           // 8 KB
  __shared__ uint64_t s_prefix;
  __shared__ uint32_t s_need;
  __shared__ uint32_t s_found;                       // 0: go on; 1: the pivot is s_prefix; 2: nothing to select
  __shared__ uint32_t s_count;

  const int tid = threadIdx.x;
  const uint32_t copy = tid & (TK_COPIES - 1);
  for (int i = tid; i < TK_BINS * TK_COPIES; i += TK_THREADS) hist[i] = 0;
  if (tid == 0) {
    s_prefix = 0;
    s_need = (uint32_t)k;
    s_found = 0;
    s_count = 0;
  }
  __syncthreads();

  for (int shift = 56; shift >= 0; shift -= 8) {
    const uint64_t prefix = s_prefix;
    if (shift < 32 && (((uint32_t)(n - 1)) >> shift) == 0) {
      // every position < n has a zero digit here, so every ~position the digit 0xff: nothing to count
      __syncthreads();
      if (tid == 0) s_prefix = prefix | (0xffull << shift);
      __syncthreads();
      continue;
    }
    // the key's two words apart: 32-bit arithmetic per score
    const uint32_t p_hi = (uint32_t)(prefix >> 32), p_lo = (uint32_t)prefix;
    if (shift >= 32) {         // a digit of ordered(overlap)
      const int s = shift - 32;
      const uint32_t mask = s == 24 ? 0u : ~0u << (s + 8);
      for_each_score(overlap, n, [&](int, uint32_t bits) {
        const uint32_t o = ordered(bits);
        if (o != 0 && (o & mask) == p_hi) atomicAdd(&hist[((o >> s) & 0xffu) * TK_COPIES + copy], 1u);
      });
    } else {                   // a digit of ~position, among the scores equal to the value already chosen
      const uint32_t mask = shift == 24 ? 0u : ~0u << (shift + 8);
      for_each_score(overlap, n, [&](int i, uint32_t bits) {
        const uint32_t q = ~(uint32_t)i;
        if (ordered(bits) == p_hi && (q & mask) == p_lo) atomicAdd(&hist[((q >> shift) & 0xffu) * TK_COPIES + copy], 1u);
      });
    }
    __syncthreads();
    if (tid < TK_BINS) {     // merge the copies (rotated start: the 32 lanes of a half-wave read 32 banks) and clear them
      uint32_t s = 0;
      for (int c = 0; c < TK_COPIES; ++c) {
        const int a = tid * TK_COPIES + ((c + tid) & (TK_COPIES - 1));
        s += hist[a];
        hist[a] = 0;
      }
      merged[tid] = s;
    }
    __syncthreads();
    if (tid < 64) {
      // lane l holds bins 255 - 4l .. 252 - 4l (descending); an inclusive scan over the lanes gives each lane the number of keys
      // in bins above its own four
      uint32_t c[4], local = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        c[j] = merged[TK_BINS - 1 - 4 * tid - j];
        local += c[j];
      }
      uint32_t incl = local;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const uint32_t o = __shfl_up(incl, off, 64);
        if (tid >= off) incl += o;
      }
      const uint32_t total = __shfl(incl, 63, 64);
      uint32_t need = s_need;
      if (shift == 56 && total < need) need = total;       // fewer than k non-NaN scores
      if (shift == 56 && total == need) {
        if (tid == 0) {
          s_found = total == 0 ? 2u : 1u;
          s_prefix = 0;
          s_need = total;
        }
      } else {
        uint32_t above = incl - local;
        if (above < need && need <= incl) {                 // exactly one lane: the digit is among its four bins
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            if (above < need && need <= above + c[j]) {
              const uint32_t d = TK_BINS - 1 - 4 * tid - j;
              const uint32_t rest = need - above;
              s_prefix = prefix | ((uint64_t)d << shift);
              s_need = rest;
              s_found = c[j] == rest ? 1u : 0u;
            }
            above += c[j];
          }
        }
      }
    }
    __syncthreads();
    if (s_found) break;
  }
  // found == 0 cannot happen (the keys are unique: the last digit's bin holds the one key still needed); s_prefix is safe anyway
  const uint32_t found = s_found;
  const uint64_t pivot = s_prefix;     // collect the keys >= pivot; 0 (fewer than k non-NaN scores) = all of them

  // 2. collect the selected keys (any order)
  if (found != 2) {
    const uint32_t p_hi = (uint32_t)(pivot >> 32), p_lo = (uint32_t)pivot;
    for_each_score(overlap, n, [&](int i, uint32_t bits) {
      const uint32_t o = ordered(bits), q = ~(uint32_t)i;
      if (o != 0 && (o > p_hi || (o == p_hi && q >= p_lo))) {
        const uint32_t slot = atomicAdd(&s_count, 1u);
        if (slot < (uint32_t)OVN_TOP_K_MAX) keys[slot] = ((uint64_t)o << 32) | q;
      }
    });
  }
  __syncthreads();
  const uint32_t cnt = min(s_count, (uint32_t)k);

  // 3. bitonic sort, descending, of the next power of two >= cnt keys (padding 0 < every valid key)
  uint32_t m = 1;
  while (m < cnt) m <<= 1;
  if ((uint32_t)tid < m && (uint32_t)tid >= cnt) keys[tid] = 0;
  for (uint32_t size = 2; size <= m; size <<= 1) {
    for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
      __syncthreads();
      const uint32_t t = tid, p = t ^ stride;
      if (t < m && p > t) {
        const uint64_t a = keys[t], b = keys[p];
        if ((t & size) == 0 ? a < b : a > b) {
          keys[t] = b;
          keys[p] = a;
        }
      }
    }
  }
  __syncthreads();

  if (tid < k) {
    i32x4 rec = {-1, 0, 0, 0};
    if ((uint32_t)tid < cnt) {
      const int pos = (int)~(uint32_t)keys[tid];
      const float v = overlap[pos];        // the element's own bits (-0 stays -0)
      rec = (i32x4){ids ? ids[pos] : pos + index_offset, __float_as_int(v), yaw ? yaw[pos] : 0, v > threshold ? 1 : 0};
    }
    reinterpret_cast<i32x4*>(out)[tid] = rec;
  }
}

}  // namespace

int ovn_top_k_forward(const float* overlap, const int32_t* yaw, const int32_t* ids, int n, int k, float threshold,
                      int index_offset, int32_t* out, hipStream_t stream) {
  hipLaunchKernelGGL(top_k_kernel<false>, dim3(1), dim3(TK_THREADS), 0, stream, overlap, yaw, ids, n, k, threshold, index_offset, out,
                     nullptr);
  OVN_HIP_CHECK(hipGetLastError());
  return OVN_OK;
}

int ovn_top_k_segments_forward(const float* overlap, const int32_t* yaw, const int32_t* ids, const int64_t* offs_dev, int B, int k,
                               float threshold, int32_t* out, hipStream_t stream) {
  if (B == 0) return OVN_OK;
  hipLaunchKernelGGL(top_k_kernel<true>, dim3(B), dim3(TK_THREADS), 0, stream, overlap, yaw, ids, 0, k, threshold, 0, out, offs_dev);
  OVN_HIP_CHECK(hipGetLastError());
  return OVN_OK;
}

namespace {

// ridx[p] = qidx[b] and pseg[p] = b, with b the last segment whose offset is <= p (the segment holding pair p: empty segments before
// it share its offset and come first).  One thread per pair, a binary search over the B + 1 offsets.
__global__ __launch_bounds__(256) void segment_ridx_kernel(const int64_t* __restrict__ offs, const int32_t* __restrict__ qidx, int B,
                                                           int n, int32_t* __restrict__ ridx, int32_t* __restrict__ pseg) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  int lo = 0, hi = B;   // offs[lo] <= p < offs[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (offs[mid] <= p) lo = mid;
    else hi = mid;
  }
  ridx[p] = qidx[lo];
  if (pseg) pseg[p] = lo;
}

}  // namespace

int ovn_segment_ridx_forward(const int64_t* offs_dev, const int32_t* qidx_dev, int B, int n, int32_t* ridx, int32_t* pseg,
                             hipStream_t stream) {
  if (n == 0) return OVN_OK;
  const unsigned blocks = (unsigned)(((int64_t)n + 255) / 256);
  hipLaunchKernelGGL(segment_ridx_kernel, dim3(blocks), dim3(256), 0, stream, offs_dev, qidx_dev, B, n, ridx, pseg);
  OVN_HIP_CHECK(hipGetLastError());
  return OVN_OK;
}
