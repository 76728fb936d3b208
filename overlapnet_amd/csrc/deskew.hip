// Motion compensation of raw LiDAR sweeps (ovn_deskew, include/ovn_hip_deskew.h): every point of a sweep moved
// into the sensor frame of one instant, under a constant twist per sweep.  The header states the arithmetic operation by operation; this
// file is built without FMA contraction so that the sequence is the one written there.
//
// One thread per point in a grid-stride loop: the host does not know the number of points (the offsets live on the device and the
// call only enqueues), so the grid is fixed and every thread reads the first and the last offset itself.  A row's scan is found by
// bisection of the offsets, which stay in cache.  16 bytes in, 16 bytes out (plus 4 of a given time) per point; no LDS, no atomics.
#include "ovn_internal.h"
#include "../../include/ovn_hip_deskew.h"

#include <cmath>

namespace {

constexpr int DESKEW_THREADS = 256;
constexpr int DESKEW_BLOCKS = 2048;          // 8 workgroups for each of the 256 CUs; further points take further trips of the loop
constexpr float DESKEW_SERIES_BELOW = 0.015625f;   // 2^-6: the header's step 3

struct DeskewArgs {
  const float4* points;
  const long long* offsets;
  const float* times;          // NULL: the azimuth route
  const double* twists;
  float4* out;
  int n_scans;
  int clockwise;
  float c0;
  float t_ref;
};

// the per-scan constants of the header, each formed in fp64 and rounded to f32 once
struct ScanMotion {
  float th, k[3], v[3], kv[3], kkv[3];
  bool copy;                   // six zeros, or a non-finite entry: the scan is copied
};

__device__ __forceinline__ void cross3(const double* a, const double* b, double* o) {
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}

__device__ __forceinline__ ScanMotion scan_motion(const double* xi) {
  ScanMotion m;
  double v[3] = {xi[0], xi[1], xi[2]}, w[3] = {xi[3], xi[4], xi[5]};
  bool zero = true, finite = true;
  for (int i = 0; i < 6; ++i) {
    zero = zero && xi[i] == 0.0;
    finite = finite && isfinite(xi[i]);
  }
  m.copy = zero || !finite;
  const double th = sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]);
  double k[3], kv[3], kkv[3];
  for (int i = 0; i < 3; ++i) k[i] = th > 0.0 ? w[i] / th : 0.0;
  cross3(k, v, kv);
  cross3(k, kv, kkv);
  m.th = (float)th;
  for (int i = 0; i < 3; ++i) {
    m.k[i] = (float)k[i];
    m.v[i] = (float)v[i];
    m.kv[i] = (float)kv[i];
    m.kkv[i] = (float)kkv[i];
  }
  return m;
}

__device__ __forceinline__ void cross3f(const float* a, const float* b, float* o) {
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}

__global__ __launch_bounds__(DESKEW_THREADS) void deskew_kernel(DeskewArgs g) {
  const long long first = g.offsets[0], last = g.offsets[g.n_scans];
  const long long stride = (long long)DESKEW_BLOCKS * DESKEW_THREADS;
  for (long long row = first + (long long)blockIdx.x * DESKEW_THREADS + threadIdx.x; row < last; row += stride) {
    // the scan: the last s with offsets[s] <= row (an empty scan shares its offset with the next and is passed over)
    int lo = 0, hi = g.n_scans;                  // offsets[lo] <= row < offsets[hi]
    while (hi - lo > 1) {
      const int mid = lo + (hi - lo) / 2;
      if (g.offsets[mid] <= row) lo = mid; else hi = mid;
    }
    const float4 p4 = g.points[row];
    const ScanMotion m = scan_motion(g.twists + (long long)lo * 6);
    if (m.copy) {
      g.out[row] = p4;
      continue;
    }
    float s;
    if (g.times) {
      s = g.times[row];
    } else {
      const float yaw = -atan2f(p4.y, p4.x);
      const float q = yaw / 3.14159274101257324f;
      const float c = 0.5f * (q + 1.0f);
      const float d = g.clockwise ? c - g.c0 : g.c0 - c;
      s = d - floorf(d);
    }
    if (!isfinite(s)) {
      g.out[row] = make_float4(0.0f, 0.0f, 0.0f, p4.w);
      continue;
    }
    const float tau = s - g.t_ref;
    const float a = tau * m.th;
    const float sa = sinf(a);
    const float sh = sinf(0.5f * a);
    const float c1 = (2.0f * sh) * sh;
    float B, Cq;
    if (fabsf(a) < DESKEW_SERIES_BELOW) {
      const float aa = a * a;
      B = a * (0.5f - aa / 24.0f);
      Cq = aa * ((1.0f / 6.0f) - aa / 120.0f);
    } else {
      B = c1 / a;
      Cq = (a - sa) / a;
    }
    const float p[3] = {p4.x, p4.y, p4.z};
    float kp[3], kkp[3], o[3];
    cross3f(m.k, p, kp);
    cross3f(m.k, kp, kkp);
    for (int i = 0; i < 3; ++i) {
      const float r = (p[i] + sa * kp[i]) + c1 * kkp[i];
      const float u = (m.v[i] + B * m.kv[i]) + Cq * m.kkv[i];
      const float t = tau * u;
      o[i] = r + t;
    }
    g.out[row] = make_float4(o[0], o[1], o[2], p4.w);
  }
}

}  // namespace

extern "C" int ovn_deskew(ovn_ctx* ctx, void* stream, const float* points_dev, const int64_t* offsets_dev, int n_scans,
                          const float* times_dev, double start_azimuth_deg, int clockwise, const double* twists_dev, double t_ref,
                          float* out_points_dev) {
  OVN_REQUIRE(ctx != nullptr, OVN_ERR_ARG, "ovn_deskew: ctx is NULL");
  OVN_REQUIRE(n_scans >= 0, OVN_ERR_ARG, "ovn_deskew: n_scans %d < 0", n_scans);
  OVN_REQUIRE(std::isfinite(t_ref) && std::isfinite((float)t_ref), OVN_ERR_ARG, "ovn_deskew: t_ref %g is not finite in float32", t_ref);
  OVN_REQUIRE(std::isfinite(start_azimuth_deg), OVN_ERR_ARG, "ovn_deskew: start_azimuth_deg %g is not finite", start_azimuth_deg);
  OVN_REQUIRE(clockwise == 0 || clockwise == 1, OVN_ERR_ARG, "ovn_deskew: clockwise %d is neither 0 nor 1", clockwise);
  if (n_scans == 0) return OVN_OK;
  OVN_REQUIRE(points_dev && offsets_dev && twists_dev && out_points_dev, OVN_ERR_ARG,
              "ovn_deskew: NULL points, offsets, twists or output");
  OVN_REQUIRE(((uintptr_t)points_dev & 15) == 0 && ((uintptr_t)out_points_dev & 15) == 0, OVN_ERR_ARG,
              "ovn_deskew: points and output must be 16-byte aligned");
  OVN_ON_DEVICE(ctx->device);
  DeskewArgs g;
  g.points = reinterpret_cast<const float4*>(points_dev);
  g.offsets = reinterpret_cast<const long long*>(offsets_dev);
  g.times = times_dev;
  g.twists = twists_dev;
  g.out = reinterpret_cast<float4*>(out_points_dev);
  g.n_scans = n_scans;
  g.clockwise = clockwise;
  g.c0 = (float)(0.5 * (start_azimuth_deg / 180.0 + 1.0));
  g.t_ref = (float)t_ref;
  hipLaunchKernelGGL(deskew_kernel, dim3(DESKEW_BLOCKS), dim3(DESKEW_THREADS), 0, (hipStream_t)stream, g);
  OVN_HIP_CHECK(hipGetLastError());
  return OVN_OK;
}
