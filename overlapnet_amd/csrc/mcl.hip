// Overlap-based Monte Carlo localization on gfx950: the particle filter around the 1-vs-U sweep (DESIGN.md 26 states every formula).
//
//   ovn_mcl_predict   motion update with Philox4x32-10 noise, particle -> map frame lookup, ascending list of the distinct frames
//   ovn_mcl_update    observation-model weights from the sweep's scores, exact power-of-two rescale, the fp64 estimate
//   ovn_mcl_resample  systematic resampling, exact in integers
//
// Per-particle arithmetic is fp32 and this file is compiled with -ffp-contract=off: a NumPy float32 restatement rounds every operation
// the same way, so the cell a position falls into is the same on both sides.  Nothing here uses an atomic: flags are plain stores of
// one value, sums run in an order fixed by the particle count alone, the resampler works on integers.  Every buffer is the caller's.
// Per-particle work (motion, weights) runs one particle per thread over the chip.  What needs an order runs where no word passes
// between workgroups: the compaction of the frame flags and the fp64 sums each in ONE 1024-thread workgroup (at most 64 particles
// per thread), the resampler one workgroup per 1024 particles, each of which adds up the integer weights below its tile itself.
#include "ovn_internal.h"

namespace {

constexpr int MCL_THREADS = 1024;
constexpr int MCL_WAVES = MCL_THREADS / 64;
constexpr int MCL_PREDICT_THREADS = 256;

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));

struct Philox {
  uint32_t w[4];
};

// Philox4x32-10 (Salmon et al., SC'11): ten rounds, the key bumped after each
__device__ __forceinline__ Philox philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
    const uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
    c0 = h1 ^ c1 ^ k0;
    c1 = l1;
    c2 = h0 ^ c3 ^ k1;
    c3 = l0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return Philox{{c0, c1, c2, c3}};
}

__device__ __forceinline__ float mcl_uniform(uint32_t k) { return ((float)(k >> 8) + 0.5f) * 0x1p-24f; }

__device__ __forceinline__ float mcl_wrap_pi(float t) {   // into (-pi, pi]
  const float PI_F = 3.14159274101257324f, TWO_PI_F = 6.28318548202514648f, INV_TWO_PI_F = 0.159154936671257019f;
  t = t - TWO_PI_F * rintf(t * INV_TWO_PI_F);
  if (t <= -PI_F) t = t + TWO_PI_F;
  if (t > PI_F) t = t - TWO_PI_F;
  return t;
}

__global__ void mcl_clear_kernel(int32_t* __restrict__ frame_slot, int M) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f < M) frame_slot[f] = -1;
}

struct MclMotion {
  float dx, dy, dth, sx, sy, sth;
  uint32_t seed_lo, seed_hi, step_lo, step_hi;
};
struct MclGrid {
  float ox, oy, inv_res;
  int nx, ny, M;
};

// one particle per thread: noise, motion, cell, frame; frame_slot[f] = 0 flags a frame somebody landed on (same value from everyone)
__global__ __launch_bounds__(MCL_PREDICT_THREADS) void mcl_predict_kernel(float* __restrict__ particles, int P, MclMotion m, MclGrid g,
                                                                          const int32_t* __restrict__ cell_frame,
                                                                          int32_t* __restrict__ particle_frame,
                                                                          int32_t* __restrict__ frame_slot) {
  const int i = blockIdx.x * MCL_PREDICT_THREADS + threadIdx.x;
  if (i >= P) return;
  f32x4 p = reinterpret_cast<const f32x4*>(particles)[i];
  const Philox r = philox4x32_10((uint32_t)i, m.step_lo, m.step_hi, 0u, m.seed_lo, m.seed_hi);
  const float TWO_PI_F = 6.28318548202514648f;
  const float rad_xy = sqrtf(-2.0f * logf(mcl_uniform(r.w[0]))), ang_xy = TWO_PI_F * mcl_uniform(r.w[1]);
  const float rad_t = sqrtf(-2.0f * logf(mcl_uniform(r.w[2]))), ang_t = TWO_PI_F * mcl_uniform(r.w[3]);
  const float zx = rad_xy * cosf(ang_xy), zy = rad_xy * sinf(ang_xy), zt = rad_t * cosf(ang_t);
  const float dx = m.dx + m.sx * zx, dy = m.dy + m.sy * zy, dth = m.dth + m.sth * zt;
  const float c = cosf(p[2]), s = sinf(p[2]);
  p[0] = p[0] + (c * dx - s * dy);
  p[1] = p[1] + (s * dx + c * dy);
  p[2] = mcl_wrap_pi(p[2] + dth);
  reinterpret_cast<f32x4*>(particles)[i] = p;
  // lookup: NaN fails every comparison, so a non-finite position is off the map
  const float fx = floorf((p[0] - g.ox) * g.inv_res), fy = floorf((p[1] - g.oy) * g.inv_res);
  int f = -1;
  if (fx >= 0.0f && fx < 2147483648.0f && fy >= 0.0f && fy < 2147483648.0f) {
    const int ix = (int)fx, iy = (int)fy;
    if (ix < g.nx && iy < g.ny) {
      f = cell_frame[(size_t)iy * g.nx + ix];
      if (f < 0 || f >= g.M) f = -1;     // an entry that names no frame counts as an empty cell
    }
  }
  particle_frame[i] = f;
  if (f >= 0) frame_slot[f] = 0;
}

__device__ __forceinline__ int wave_inclusive_sum(int v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int t = __shfl_up(v, off, 64);
    if (lane >= off) v += t;
  }
  return v;
}

// ONE workgroup: flags -> ascending frame_list, frame_slot; particles off the map counted; the 16-byte record
__global__ __launch_bounds__(MCL_THREADS) void mcl_compact_kernel(const int32_t* __restrict__ particle_frame, int P,
                                                                  int32_t* __restrict__ frame_slot, int M,
                                                                  int32_t* __restrict__ frame_list, int32_t* __restrict__ record) {
  __shared__ int wsum[MCL_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int base = 0;
  for (int f0 = 0; f0 < M; f0 += MCL_THREADS) {
    const int f = f0 + tid;
    const int flag = (f < M && frame_slot[f] == 0) ? 1 : 0;
    const int incl = wave_inclusive_sum(flag);
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < MCL_WAVES; ++w) {
      const int s = wsum[w];
      before += w < wave ? s : 0;
      total += s;
    }
    const int pos = base + before + incl - flag;
    if (f < M) {
      frame_slot[f] = flag ? pos : -1;
      if (flag) frame_list[pos] = f;
    }
    base += total;
    __syncthreads();      // wsum is rewritten by the next tile
  }
  int off = 0;
  for (int i = tid; i < P; i += MCL_THREADS) off += particle_frame[i] < 0 ? 1 : 0;
  off = wave_inclusive_sum(off);
  if (lane == 63) wsum[wave] = off;
  __syncthreads();
  if (tid == 0) {
    int total = 0;
    for (int w = 0; w < MCL_WAVES; ++w) total += wsum[w];
    // ONE 16-byte store: a host that polls word 3 of a record in pinned host memory sees the four words appear together
    *reinterpret_cast<i32x4*>(record) = (i32x4){base, total, 0, 1};
  }
}

struct MclBest {
  float v;
  int k;
};
__device__ __forceinline__ MclBest mcl_better(MclBest a, MclBest b) {   // larger weight wins, equal weights: the smaller position
  if (b.k < 0) return a;
  if (a.k < 0) return b;
  if (b.v > a.v || (b.v == a.v && b.k < a.k)) return b;
  return a;
}

// sin and cos of a heading |t| <= 4 in fp64, to 1e-14: t = k pi / 2 + y with |y| <= pi / 4 (+ 1e-16 of slack), Taylor polynomials of
// degree 15 and 16 in y (truncation (pi / 4)^17 / 17! = 5e-17), then the quadrant.  The library sincos() pays for arguments of any
// size; here it was most of the estimate's time (64 headings per thread in one workgroup).
__device__ __forceinline__ void mcl_sincos(double t, double& sn, double& cs) {
  const double k = rint(t * 0.63661977236758134308);                  // 2 / pi
  const double y = fma(-k, 6.12323399573676603587e-17, fma(-k, 1.57079632679489655800, t));   // pi / 2 = hi + lo
  const double z = y * y;
  double s = -7.6471637318198164759e-13;                              // -1 / 15!
  s = fma(s, z, 1.6059043836821614599e-10);                           //  1 / 13!
  s = fma(s, z, -2.5052108385441718775e-08);                          // -1 / 11!
  s = fma(s, z, 2.7557319223985890653e-06);                           //  1 / 9!
  s = fma(s, z, -1.9841269841269841270e-04);                          // -1 / 7!
  s = fma(s, z, 8.3333333333333333333e-03);                           //  1 / 5!
  s = fma(s, z, -1.6666666666666666667e-01);                          // -1 / 3!
  s = fma(s * z, y, y);
  double c = 4.7794773323873852974e-14;                               //  1 / 16!
  c = fma(c, z, -1.1470745597729724714e-11);                          // -1 / 14!
  c = fma(c, z, 2.0876756987868098979e-09);                           //  1 / 12!
  c = fma(c, z, -2.7557319223985890653e-07);                          // -1 / 10!
  c = fma(c, z, 2.4801587301587301587e-05);                           //  1 / 8!
  c = fma(c, z, -1.3888888888888888889e-03);                          // -1 / 6!
  c = fma(c, z, 4.1666666666666666667e-02);                           //  1 / 4!
  c = fma(c, z, -0.5);
  c = fma(c, z, 1.0);
  const int q = (int)k & 3;                                           // k in -3 .. 3
  sn = (q & 1) ? c : s;
  cs = (q & 1) ? s : c;
  if (q == 1 || q == 2) cs = -cs;
  if (q == 2 || q == 3) sn = -sn;
}

struct MclObs {
  float sigma, eps, one_minus_eps, o_min;
};

// thread t sums its particles t, t + 1024, ... in that order, a wave folds its 64 lanes by halving, thread 0 adds the 16 wave sums in
// wave order: the order depends on P alone
template <int N>
__device__ __forceinline__ void mcl_block_sum(double (&v)[N], double (*red)[N], double (&out)[N]) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = v[k] + __shfl_down(v[k], off, 64);
  if ((threadIdx.x & 63) == 0)
#pragma unroll
    for (int k = 0; k < N; ++k) red[threadIdx.x >> 6][k] = v[k];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < N; ++k) {
    double s = red[0][k];
    for (int w = 1; w < MCL_WAVES; ++w) s = s + red[w][k];
    out[k] = s;
  }
  __syncthreads();        // red may be reused
}

// one particle per thread, any number of workgroups: w <- the product w o g (the chain frame -> slot -> score is three dependent loads
// per particle; spread over the chip it costs a few microseconds, inside the one-workgroup kernel below it was most of its time)
__global__ __launch_bounds__(MCL_PREDICT_THREADS) void mcl_weight_kernel(float* __restrict__ particles, int P,
                                                                         const int32_t* __restrict__ particle_frame,
                                                                         const int32_t* __restrict__ frame_slot,
                                                                         const float* __restrict__ frame_yaw, int M,
                                                                         const float* __restrict__ overlap,
                                                                         const int32_t* __restrict__ yaw, int U, MclObs ob) {
  const int i = blockIdx.x * MCL_PREDICT_THREADS + threadIdx.x;
  if (i >= P) return;
  const float RAD2DEG_F = 57.2957801818847656f;
  const f32x4 p = reinterpret_cast<const f32x4*>(particles)[i];
  const int f = particle_frame[i];
  int slot = -1;
  if (f >= 0 && f < M) {
    slot = frame_slot[f];
    if (slot >= U) slot = -1;
  }
  float prod;
  if (slot >= 0) {
    const float of = overlap[slot];
    const float o = of > ob.o_min ? of : ob.o_min;            // a NaN score gives o_min
    float d = (p[2] - frame_yaw[f]) * RAD2DEG_F - (float)yaw[slot];
    d = d - 360.0f * rintf(d / 360.0f);
    const float t = d / ob.sigma;
    const float gy = ob.eps + ob.one_minus_eps * expf(-0.5f * (t * t));
    prod = (p[3] * o) * gy;
  } else {
    prod = (p[3] * ob.o_min) * ob.eps;
  }
  particles[4 * (size_t)i + 3] = prod;
}

// ONE workgroup: the products' maximum, the exact rescale, the estimate
__global__ __launch_bounds__(MCL_THREADS) void mcl_estimate_kernel(float* __restrict__ particles, int P,
                                                                   const int32_t* __restrict__ particle_frame,
                                                                   const int32_t* __restrict__ frame_slot, int M, int U,
                                                                   double* __restrict__ estimate, double* __restrict__ spread) {
  __shared__ float smax[MCL_WAVES];
  __shared__ int scnt[MCL_WAVES];
  __shared__ float sbv[MCL_WAVES];
  __shared__ int sbk[MCL_WAVES];
  __shared__ double red[MCL_WAVES][6];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float vmax = 0.0f;
  int on_map = 0;
#pragma unroll 4
  for (int i = tid; i < P; i += MCL_THREADS) {          // (no branch around a load: the iterations' loads overlap)
    const float prod = particles[4 * (size_t)i + 3];
    const int f = particle_frame[i];
    const bool in = f >= 0 && f < M;
    const int slot = frame_slot[in ? f : 0];
    on_map += (in && slot >= 0 && slot < U) ? 1 : 0;
    if (prod > vmax && prod < INFINITY) vmax = prod;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    vmax = fmaxf(vmax, __shfl_down(vmax, off, 64));
    on_map += __shfl_down(on_map, off, 64);
  }
  if (lane == 0) {
    smax[wave] = vmax;
    scnt[wave] = on_map;
  }
  __syncthreads();
  vmax = smax[0];
  on_map = scnt[0];
  for (int w = 1; w < MCL_WAVES; ++w) {
    vmax = fmaxf(vmax, smax[w]);
    on_map += scnt[w];
  }
  if (!(vmax > 0.0f)) {                    // no finite positive product: the weights stay the products
    if (tid == 0) {
      f64x2* e = reinterpret_cast<f64x2*>(estimate);
      e[0] = (f64x2){1.0, 0.0};
      e[1] = (f64x2){0.0, 0.0};
      e[2] = (f64x2){0.0, 0.0};
      e[3] = (f64x2){-1.0, (double)on_map};
      if (spread) *spread = 0.0;
    }
    return;
  }
  int e2 = 0;
  (void)frexpf(vmax, &e2);
  double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};     // w, w^2, w x, w y, w sin, w cos
  MclBest best = {0.0f, -1};
  for (int i = tid; i < P; i += MCL_THREADS) {
    const f32x4 p = reinterpret_cast<const f32x4*>(particles)[i];
    const float wf = ldexpf(p[3], -e2);
    particles[4 * (size_t)i + 3] = wf;
    const double w = (double)wf, th = (double)p[2];
    acc[0] = acc[0] + w;
    acc[1] = acc[1] + w * w;
    acc[2] = acc[2] + w * (double)p[0];
    acc[3] = acc[3] + w * (double)p[1];
    double sn, cs;
    mcl_sincos(th, sn, cs);        // (a heading outside [-4, 4] -- the contract is (-pi, pi] -- only loses accuracy)
    acc[4] = acc[4] + w * sn;
    acc[5] = acc[5] + w * cs;
    if (wf == wf) best = mcl_better(best, MclBest{wf, i});
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    MclBest o;
    o.v = __shfl_down(best.v, off, 64);
    o.k = __shfl_down(best.k, off, 64);
    best = mcl_better(best, o);
  }
  if (lane == 0) {
    sbv[wave] = best.v;
    sbk[wave] = best.k;
  }
  double sum[6];
  mcl_block_sum<6>(acc, red, sum);       // (its first barrier also publishes sbv / sbk)
  const double xm = sum[2] / sum[0], ym = sum[3] / sum[0];
  if (tid == 0) {
    for (int w = 1; w < MCL_WAVES; ++w) best = mcl_better(best, MclBest{sbv[w], sbk[w]});
    f64x2* e = reinterpret_cast<f64x2*>(estimate);
    e[0] = (f64x2){0.0, sum[0]};
    e[1] = (f64x2){(sum[0] * sum[0]) / sum[1], xm};
    e[2] = (f64x2){ym, atan2(sum[4], sum[5])};
    e[3] = (f64x2){(double)best.k, (double)on_map};
  }
  if (spread) {                            // weighted rms distance from the mean position, same summation order
    double a2[1] = {0.0};
    for (int i = tid; i < P; i += MCL_THREADS) {
      const f32x4 p = reinterpret_cast<const f32x4*>(particles)[i];
      const double ex = (double)p[0] - xm, ey = (double)p[1] - ym;
      a2[0] = a2[0] + (double)p[3] * (ex * ex + ey * ey);
    }
    double s2[1];
    mcl_block_sum<1>(a2, reinterpret_cast<double(*)[1]>(&red[0][0]), s2);
    if (tid == 0) *spread = sqrt(s2[0] / sum[0]);
  }
}

__device__ __forceinline__ uint64_t mcl_quantum(float w) {     // floor(w 2^30); 0 for negative / non-finite; weights >= 1 saturate
  if (!(w > 0.0f) || !(w < INFINITY)) return 0;
  if (w >= 1.0f) return (1ull << 30) - 1;
  return (uint64_t)(w * 0x1p30f);
}

// number of outputs j in [0, n_out) with j S + r < c n_out: min(n_out, ceil((c n_out - r) / S)), exactly.  The quotient is at most
// n_out <= 2^16 and both factors of the fp64 estimate carry a relative error of 2^-53, so the estimate is within 1 of the floor; two
// integer comparisons make it the ceiling (v S < 2^63: v <= 2^16 + 1, S < 2^46)
__device__ __forceinline__ int mcl_first(uint64_t c, uint64_t S, uint64_t r, int n_out, double inv_s) {
  const uint64_t x = c * (uint64_t)n_out;
  if (x <= r) return 0;
  const uint64_t d = x - r;
  uint64_t v = (uint64_t)((double)d * inv_s);
  while (v * S < d) ++v;
  while (v > 0 && (v - 1) * S >= d) --v;
  return v < (uint64_t)n_out ? (int)v : n_out;
}

__device__ __forceinline__ void mcl_emit(float* __restrict__ out, int32_t* __restrict__ ancestor, int j, float x, float y, float th, int a) {
  reinterpret_cast<f32x4*>(out)[j] = (f32x4){x, y, th, 1.0f};
  ancestor[j] = a;
}

constexpr int MCL_SHORT_RUN = 4;       // a lane writes a run of up to this many copies itself; its wave writes a longer one together

// One workgroup per tile of 1024 particles (thread t of workgroup k takes particle 1024 k + t), and no word passes between workgroups:
// each adds up ALL the quanta itself (S) and, on the way, those below its tile (its carry) -- 4 bytes per particle from L2, integer
// sums, so every workgroup gets the same S.  Then it scans its tile (wave scan, 16 wave sums through LDS), which gives particle a its
// C[a - 1] and C[a] and so the run of outputs [first(C[a - 1]), first(C[a])) that copy it; the runs of all tiles tile [0, n_out).
// Short runs are written by their lane, a long one by the 64 lanes of its wave, so one dominant particle costs n_out / 64 steps, not
// n_out.  Workgroup 0 writes the record.
__global__ __launch_bounds__(MCL_THREADS) void mcl_resample_kernel(const float* __restrict__ particles, int P, uint32_t seed_lo,
                                                                   uint32_t seed_hi, uint32_t step_lo, uint32_t step_hi,
                                                                   float* __restrict__ out, int n_out, int32_t* __restrict__ ancestor,
                                                                   int32_t* __restrict__ record) {
  __shared__ uint64_t wsum[2][MCL_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int a = blockIdx.x * MCL_THREADS + tid;
  const f32x4 none = {0.0f, 0.0f, 0.0f, 0.0f};
  const f32x4 p = a < P ? reinterpret_cast<const f32x4*>(particles)[a] : none;
  uint64_t all = 0, below = 0;
#pragma unroll 4
  for (int i = tid; i < P; i += MCL_THREADS) {
    const uint64_t qi = mcl_quantum(particles[4 * (size_t)i + 3]);
    all += qi;
    below += i < (int)(blockIdx.x * MCL_THREADS) ? qi : 0;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    all += __shfl_down(all, off, 64);
    below += __shfl_down(below, off, 64);
  }
  const uint64_t q = a < P ? mcl_quantum(p[3]) : 0;
  uint64_t incl = q;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint64_t t = __shfl_up(incl, off, 64);
    if (lane >= off) incl += t;
  }
  if (lane == 0) {
    wsum[0][wave] = all;
    wsum[1][wave] = below;
  }
  __syncthreads();
  uint64_t S = 0, carry = 0;
#pragma unroll
  for (int w = 0; w < MCL_WAVES; ++w) {
    S += wsum[0][w];
    carry += wsum[1][w];
  }
  if (S == 0) {                             // nothing to draw from: nothing is written but the record
    if (blockIdx.x == 0 && tid == 0) *reinterpret_cast<i32x4*>(record) = (i32x4){1, 0, 0, 1};
    return;
  }
  __syncthreads();                          // wsum[0] is rewritten with the tile's wave sums
  if (lane == 63) wsum[0][wave] = incl;
  __syncthreads();
#pragma unroll
  for (int w = 0; w < MCL_WAVES; ++w) carry += w < wave ? wsum[0][w] : 0;
  const Philox ph = philox4x32_10(0u, step_lo, step_hi, 1u, seed_lo, seed_hi);
  const uint64_t r = ((uint64_t)ph.w[0] | ((uint64_t)ph.w[1] << 32)) % S;
  const double inv_s = 1.0 / (double)S;
  const uint64_t c1 = carry + incl;
  int j0 = 0, j1 = 0;
  if (q != 0) {
    j0 = mcl_first(c1 - q, S, r, n_out, inv_s);
    j1 = mcl_first(c1, S, r, n_out, inv_s);
  }
  const int len = j1 - j0;
  if (len <= MCL_SHORT_RUN)
    for (int j = j0; j < j1; ++j) mcl_emit(out, ancestor, j, p[0], p[1], p[2], a);
  unsigned long long longs = __ballot(len > MCL_SHORT_RUN);
  while (longs) {                           // (wave-uniform)
    const int l = __ffsll((long long)longs) - 1;
    longs &= longs - 1;
    const int b0 = __shfl(j0, l, 64), b1 = __shfl(j1, l, 64), ba = __shfl(a, l, 64);
    const float bx = __shfl(p[0], l, 64), by = __shfl(p[1], l, 64), bt = __shfl(p[2], l, 64);
    for (int j = b0 + lane; j < b1; j += 64) mcl_emit(out, ancestor, j, bx, by, bt, ba);
  }
  if (blockIdx.x == 0 && tid == 0) *reinterpret_cast<i32x4*>(record) = (i32x4){0, n_out, 0, 1};
}

}  // namespace

int ovn_mcl_predict_forward(float* particles, int P, const double* motion6, uint64_t seed, uint64_t step, const int32_t* cell_frame,
                            double origin_x, double origin_y, double resolution, int nx, int ny, int M, int32_t* particle_frame,
                            int32_t* frame_slot, int32_t* frame_list, int32_t* record, hipStream_t stream) {
  MclMotion m;
  m.dx = (float)motion6[0];
  m.dy = (float)motion6[1];
  m.dth = (float)motion6[2];
  m.sx = (float)motion6[3];
  m.sy = (float)motion6[4];
  m.sth = (float)motion6[5];
  m.seed_lo = (uint32_t)seed;
  m.seed_hi = (uint32_t)(seed >> 32);
  m.step_lo = (uint32_t)step;
  m.step_hi = (uint32_t)(step >> 32);
  MclGrid g;
  g.ox = (float)origin_x;
  g.oy = (float)origin_y;
  g.inv_res = (float)(1.0 / resolution);
  g.nx = nx;
  g.ny = ny;
  g.M = M;
  hipLaunchKernelGGL(mcl_clear_kernel, dim3((M + 255) / 256), dim3(256), 0, stream, frame_slot, M);
  hipLaunchKernelGGL(mcl_predict_kernel, dim3((P + MCL_PREDICT_THREADS - 1) / MCL_PREDICT_THREADS), dim3(MCL_PREDICT_THREADS), 0,
                     stream, particles, P, m, g, cell_frame, particle_frame, frame_slot);
  hipLaunchKernelGGL(mcl_compact_kernel, dim3(1), dim3(MCL_THREADS), 0, stream, particle_frame, P, frame_slot, M, frame_list, record);
  OVN_HIP_CHECK(hipGetLastError());
  return OVN_OK;
}

int ovn_mcl_update_forward(float* particles, int P, const int32_t* particle_frame, const int32_t* frame_slot, const float* frame_yaw,
                           int M, const float* overlap, const int32_t* yaw, int U, double sigma_yaw, double eps_yaw, double overlap_min,
                           double* estimate, double* spread, hipStream_t stream) {
  MclObs ob;
  ob.sigma = (float)sigma_yaw;
  ob.eps = (float)eps_yaw;
  ob.one_minus_eps = 1.0f - ob.eps;
  ob.o_min = (float)overlap_min;
  hipLaunchKernelGGL(mcl_weight_kernel, dim3((P + MCL_PREDICT_THREADS - 1) / MCL_PREDICT_THREADS), dim3(MCL_PREDICT_THREADS), 0, stream,
                     particles, P, particle_frame, frame_slot, frame_yaw, M, overlap, yaw, U, ob);
  hipLaunchKernelGGL(mcl_estimate_kernel, dim3(1), dim3(MCL_THREADS), 0, stream, particles, P, particle_frame, frame_slot, M, U, estimate,
                     spread);
  OVN_HIP_CHECK(hipGetLastError());
  return OVN_OK;
}

int ovn_mcl_resample_forward(const float* particles, int P, uint64_t seed, uint64_t step, float* out, int n_out, int32_t* ancestor,
                             int32_t* record, hipStream_t stream) {
  hipLaunchKernelGGL(mcl_resample_kernel, dim3((P + MCL_THREADS - 1) / MCL_THREADS), dim3(MCL_THREADS), 0, stream, particles, P, (uint32_t)seed, (uint32_t)(seed >> 32),
                     (uint32_t)step, (uint32_t)(step >> 32), out, n_out, ancestor, record);
  OVN_HIP_CHECK(hipGetLastError());
  return OVN_OK;
}
