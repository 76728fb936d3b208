// Data-parallel training on gfx950: the ranks' gradients reduced and Adagrad applied in one pass (ovn_grad_reduce_adagrad).
//
// G is (world, stride) float32, row r the flat gradient of rank r; w[r] = n_r / n (fp64, host) the share of the global batch rank r
// held.  For every element i < count:
//     s = 0.0;  for r = 0 .. world - 1 in this order, rows with w[r] == 0 skipped (and not read):  s = s + w[r] * (double)G[r][i]
//     g = (float)s                                              rounded once
//     a = accum[i] + g * g;  accum[i] = a                       Keras 2.1.5's Adagrad (train.adagrad_step)
//     params[i] = params[i] - (lr * g) / (sqrtf(a) + eps)
// Every operation is one correctly rounded IEEE operation: this file is compiled with -ffp-contract=off (no FMA is formed from
// w * G + s, g * g + a), hipcc's default fp32 divide and sqrt are the correctly rounded expansions, and the kernel mode keeps fp32
// denormals, so the result is the bits of the NumPy restatement in tests/_grad_reduce_ref.py.  No atomics and a fixed order: the
// same bits on every rank and every run, whatever order the collective delivered the rows in.
//
// Memory-bound: 4 * (rows read) + 8 bytes in, 8 - 12 bytes out per element, nothing reused, so no LDS.  One thread takes four
// consecutive elements with 16-byte loads and stores where all four exist (and every buffer is 16-byte aligned: the row stride is
// a multiple of 4 floats), the last 1 - 3 elements go one by one; a grid-stride loop with 64-bit indices covers any count.
#include <algorithm>
#include <cmath>

#include "ovn_internal.h"

namespace {

constexpr int GR_THREADS = 256;
constexpr int GR_MAX_BLOCKS = 2048;        // 256 CUs x 8 workgroups: the rest of a large buffer is walked by the grid-stride loop

struct GrWeights {
  double w[OVN_GRAD_REDUCE_MAX_WORLD];     // 512 bytes of kernel arguments: read through the scalar cache, uniform for the launch
};

// one Adagrad update: a <- a + g g, returns p - (lr g) / (sqrt(a) + eps); five fp32 operations, each rounded on its own
__device__ __forceinline__ float gr_update(float g, float& a, float p, float lr, float eps) {
  const float gg = g * g;
  a = a + gg;
  const float num = lr * g;
  const float den = sqrtf(a) + eps;
  return p - num / den;
}

template <bool UPDATE>
__device__ __forceinline__ void gr_finish(double s, int64_t i, float* __restrict__ params, float* __restrict__ accum, float lr, float eps,
                                          float* __restrict__ grad_out) {
  const float g = (float)s;
  if (grad_out) grad_out[i] = g;
  if constexpr (UPDATE) {
    float a = accum[i];
    params[i] = gr_update(g, a, params[i], lr, eps);
    accum[i] = a;
  }
}

// VEC: every buffer is 16-byte aligned, so quads take 16-byte accesses; otherwise every element goes through the scalar form
template <bool UPDATE, bool VEC>
__global__ __launch_bounds__(GR_THREADS) void grad_reduce_adagrad_kernel(const float* __restrict__ G, int world, int64_t stride,
                                                                         GrWeights rw, int64_t count, float* __restrict__ params,
                                                                         float* __restrict__ accum, float lr, float eps,
                                                                         float* __restrict__ grad_out) {
  const int64_t nquad = (count + 3) >> 2;
  const int64_t step = (int64_t)gridDim.x * GR_THREADS;
  for (int64_t q = (int64_t)blockIdx.x * GR_THREADS + threadIdx.x; q < nquad; q += step) {
    const int64_t i0 = q << 2;
    if (VEC && i0 + 3 < count) {
      double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
      for (int r = 0; r < world; ++r) {
        const double w = rw.w[r];
        if (w == 0.0) continue;            // uniform: a rank that held no pair sends a row nobody reads
        const f32x4 v = *reinterpret_cast<const f32x4*>(G + (int64_t)r * stride + i0);
        s0 = s0 + w * (double)v.x;
        s1 = s1 + w * (double)v.y;
        s2 = s2 + w * (double)v.z;
        s3 = s3 + w * (double)v.w;
      }
      const f32x4 g = {(float)s0, (float)s1, (float)s2, (float)s3};
      if (grad_out) *reinterpret_cast<f32x4*>(grad_out + i0) = g;
      if constexpr (UPDATE) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(accum + i0);
        f32x4 p = *reinterpret_cast<const f32x4*>(params + i0);
        float a0 = a.x, a1 = a.y, a2 = a.z, a3 = a.w;
        p.x = gr_update(g.x, a0, p.x, lr, eps);
        p.y = gr_update(g.y, a1, p.y, lr, eps);
        p.z = gr_update(g.z, a2, p.z, lr, eps);
        p.w = gr_update(g.w, a3, p.w, lr, eps);
        *reinterpret_cast<f32x4*>(accum + i0) = (f32x4){a0, a1, a2, a3};
        *reinterpret_cast<f32x4*>(params + i0) = p;
      }
    } else {
      const int64_t i1 = i0 + 4 < count ? i0 + 4 : count;
      for (int64_t i = i0; i < i1; ++i) {
        double s = 0.0;
        for (int r = 0; r < world; ++r) {
          const double w = rw.w[r];
          if (w == 0.0) continue;
          s = s + w * (double)G[(int64_t)r * stride + i];
        }
        gr_finish<UPDATE>(s, i, params, accum, lr, eps, grad_out);
      }
    }
  }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

int ovn_grad_reduce_adagrad(ovn_ctx* ctx, const float* grads_dev, int world, int64_t stride, const double* rank_weight_host,
                            int64_t count, float* params_dev, float* accum_dev, float lr, float eps, float* grad_out_dev,
                            void* stream_) {
  OVN_REQUIRE(world >= 1 && world <= OVN_GRAD_REDUCE_MAX_WORLD, OVN_ERR_ARG, "ovn_grad_reduce_adagrad: world %d outside 1..%d", world,
              OVN_GRAD_REDUCE_MAX_WORLD);
  OVN_REQUIRE(count >= 1, OVN_ERR_ARG, "ovn_grad_reduce_adagrad: count %lld < 1", (long long)count);
  OVN_REQUIRE(stride >= count && (stride & 3) == 0, OVN_ERR_ARG,
              "ovn_grad_reduce_adagrad: stride %lld must be a multiple of 4 and at least count %lld", (long long)stride, (long long)count);
  OVN_REQUIRE(std::isfinite(lr) && std::isfinite(eps) && eps >= 0.f, OVN_ERR_ARG,
              "ovn_grad_reduce_adagrad: lr and eps must be finite, eps >= 0 (lr %g, eps %g)", (double)lr, (double)eps);
  OVN_REQUIRE((params_dev == nullptr) == (accum_dev == nullptr), OVN_ERR_ARG,
              "ovn_grad_reduce_adagrad: params and accum are given together or not at all");
  OVN_REQUIRE(params_dev || grad_out_dev, OVN_ERR_ARG, "ovn_grad_reduce_adagrad: no output (params / accum and grad_out all NULL)");
  OVN_REQUIRE(rank_weight_host, OVN_ERR_ARG, "ovn_grad_reduce_adagrad: NULL argument");
  GrWeights rw;
  bool any = false;
  for (int r = 0; r < OVN_GRAD_REDUCE_MAX_WORLD; ++r) {
    rw.w[r] = r < world ? rank_weight_host[r] : 0.0;
    OVN_REQUIRE(std::isfinite(rw.w[r]) && rw.w[r] >= 0.0, OVN_ERR_ARG, "ovn_grad_reduce_adagrad: weight %g of rank %d is negative or not finite",
                rw.w[r], r);
    any = any || rw.w[r] != 0.0;
  }
  OVN_REQUIRE(any, OVN_ERR_ARG, "ovn_grad_reduce_adagrad: every rank weight is zero");
  OVN_REQUIRE(ctx && grads_dev, OVN_ERR_ARG, "ovn_grad_reduce_adagrad: NULL argument");
  OVN_ON_DEVICE(ctx->device);
  hipStream_t stream = (hipStream_t)stream_;
  const int64_t nquad = (count + 3) >> 2;
  const unsigned blocks = (unsigned)std::min<int64_t>((nquad + GR_THREADS - 1) / GR_THREADS, GR_MAX_BLOCKS);
  const bool vec = aligned16(grads_dev) && aligned16(params_dev) && aligned16(accum_dev) && aligned16(grad_out_dev);
  OvnProfScope ps(ctx, OVN_K_LEG, stream);
  if (params_dev) {
    if (vec)
      hipLaunchKernelGGL((grad_reduce_adagrad_kernel<true, true>), dim3(blocks), dim3(GR_THREADS), 0, stream, grads_dev, world, stride, rw,
                         count, params_dev, accum_dev, lr, eps, grad_out_dev);
    else
      hipLaunchKernelGGL((grad_reduce_adagrad_kernel<true, false>), dim3(blocks), dim3(GR_THREADS), 0, stream, grads_dev, world, stride, rw,
                         count, params_dev, accum_dev, lr, eps, grad_out_dev);
  } else {
    if (vec)
      hipLaunchKernelGGL((grad_reduce_adagrad_kernel<false, true>), dim3(blocks), dim3(GR_THREADS), 0, stream, grads_dev, world, stride, rw,
                         count, params_dev, accum_dev, lr, eps, grad_out_dev);
    else
      hipLaunchKernelGGL((grad_reduce_adagrad_kernel<false, false>), dim3(blocks), dim3(GR_THREADS), 0, stream, grads_dev, world, stride,
                         rw, count, params_dev, accum_dev, lr, eps, grad_out_dev);
  }
  OVN_HIP_CHECK(hipGetLastError());
  return OVN_OK;
}
