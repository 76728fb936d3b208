// Loop-closure verification on gfx950: projective point-to-plane ICP on the range images ovn_project writes, one launch for a batch
// of (source scan, target scan, initial pose) pairs.
//
// One 512-thread workgroup per pair stays resident through all `iterations + 1` passes; the pose (fp64) lives in LDS.  A pass:
//   1. every thread walks its fixed, strided set of source pixels -- group g = tid + k * 512 holds pixels 4g .. 4g + 3, read with
//      16-byte loads (range: 1, vertex: 4, normal: 3) -- and for each pixel with range > 0 moves the point by the current pose,
//      projects it into the target image (range_projection's formulas, plain fp32 atan2f / asinf), gathers the target's vertex and
//      normal there (the gathers of a group's four points are issued together), applies the gates and adds w J^T J (21 unique
//      entries), w J^T r (6), w r^2, the inlier count and the count of valid source pixels to 30 accumulators in registers
//      (per-point arithmetic fp32, every sum fp64);
//   2. a fixed tree reduces them: __shfl_down inside the wave (32, 16, .. 1), one LDS row per wave, then 30 threads add the 8 rows
//      in order.  No atomics: the order of every sum depends on (H, W) and the block size alone, so a pair's outputs have the same
//      bits alone or in any batch, at any position, run after run;
//   3. thread 0 solves A xi = -b (6x6 Cholesky, fp64) and updates T <- exp(xi) T with the closed-form SE(3) exponential; a barrier
//      hands the new pose to everybody.
// The last pass has no solve: its sums describe the pose that is returned (inliers, rms).  A pass with fewer than min_inliers
// correspondences, a non-positive or non-finite pivot, a non-finite step or a non-finite updated pose stops the pair: status 1, the
// pose it had before that pass (T0 bit for bit when no step was taken) and that pass's own sums as the statistics -- they were
// taken at the returned pose too.
// Every comparison is written so that a NaN in the input drops the point: nothing non-finite reaches the sums, and a pose is
// committed only if it is finite.  (A T0 that holds a NaN or Inf therefore matches no point and comes back as it is, status 1.)
//
// Compiled without FMA contraction (csrc/Makefile): the two instantiations below then round alike, and a pair gives the same bits
// from aligned and unaligned maps.
//
// With the query as the target of all its candidates the k workgroups gather from the same 1.8 MB (64 x 900) in cache; the source
// reads are linear.
#include "ovn_internal.h"

namespace {

constexpr int ICP_THREADS = 512;
constexpr int ICP_WAVES = ICP_THREADS / 64;
constexpr int ICP_A = 21, ICP_B = 6;
constexpr int ICP_E = ICP_A + ICP_B;        // 27: sum of w r^2
constexpr int ICP_COUNT = ICP_E + 1;        // 28: correspondences that passed every gate
constexpr int ICP_VALID = ICP_COUNT + 1;    // 29: source pixels with range > 0
constexpr int ICP_SUMS = ICP_VALID + 1;     // 30
constexpr int ICP_ACC = ICP_COUNT;          // the first 28 are fp64 accumulators; the two counts are integers until the reduction

struct IcpArgs {
  const float* vertex;
  const float* normal;
  const float* range;
  int n_scans, H, W;
  float fov_down_abs, inv_fov, max_range;   // radians; 1 / (|fov_up| + |fov_down|)
  const int32_t* src_idx;
  const int32_t* tgt_idx;
  const double* init_pose;
  int iterations;
  float max_dist2, cos_min, huber;
  int min_inliers;
  double* pose;
  double* stats;
  double* system;
};

struct IcpPose {
  float r[9], t[3];
};

// A source point in three steps, so that the four points of a group have their target gathers in flight together: a pass of one
// workgroup is bound by the latency of dependent loads, not by their number.
struct IcpPoint {
  float x, y, z;       // p' = R p + t
  float mx, my, mz;    // R n_s
  int pix;             // target pixel, 0 when !ok (a safe address: nothing of it is used)
  bool ok;
};

// 1. move the point, project it: everything that needs no target data
__device__ __forceinline__ IcpPoint icp_project(const IcpArgs& a, const IcpPose& T, bool valid, float px, float py, float pz, float sx,
                                                float sy, float sz) {
  IcpPoint P;
  P.x = T.r[0] * px + T.r[1] * py + T.r[2] * pz + T.t[0];
  P.y = T.r[3] * px + T.r[4] * py + T.r[5] * pz + T.t[1];
  P.z = T.r[6] * px + T.r[7] * py + T.r[8] * pz + T.t[2];
  P.mx = T.r[0] * sx + T.r[1] * sy + T.r[2] * sz;
  P.my = T.r[3] * sx + T.r[4] * sy + T.r[5] * sz;
  P.mz = T.r[6] * sx + T.r[7] * sy + T.r[8] * sz;
  const float d = sqrtf(P.x * P.x + P.y * P.y + P.z * P.z);
  bool ok = valid && d > 0.0f && d < a.max_range;
  const float yaw = -atan2f(P.y, P.x);
  const float pitch = asinf(fminf(fmaxf(P.z / d, -1.0f), 1.0f));
  const float uf = floorf(0.5f * (yaw * 0.318309886183790672f + 1.0f) * (float)a.W);
  const float vf = floorf((1.0f - (pitch + a.fov_down_abs) * a.inv_fov) * (float)a.H);
  ok = ok && vf >= 0.0f && vf < (float)a.H;                   // outside the vertical field of view (or NaN): no correspondence
  ok = ok && uf >= 0.0f;                                      // NaN only: yaw is in [-pi, pi]
  ok = ok && sx * sx + sy * sy + sz * sz < 1.5f;              // no normal at the source pixel
  P.ok = ok;
  P.pix = ok ? (int)vf * a.W + min((int)uf, a.W - 1) : 0;
  return P;
}

// 3. gates, residual, weight, and the point's row into acc / cnt (q, n, rq: the target's vertex, normal and range at P.pix)
__device__ __forceinline__ void icp_accumulate(const IcpArgs& a, const IcpPoint& P, float qx, float qy, float qz, float nx, float ny,
                                               float nz, float rq, double (&acc)[ICP_ACC], int& cnt) {
  const float dx = P.x - qx, dy = P.y - qy, dz = P.z - qz;
  bool ok = P.ok && rq > 0.0f;
  ok = ok && nx * nx + ny * ny + nz * nz < 1.5f;              // -1 -1 -1: no normal at the target pixel
  ok = ok && dx * dx + dy * dy + dz * dz <= a.max_dist2;
  ok = ok && nx * P.mx + ny * P.my + nz * P.mz >= a.cos_min;
  if (!ok) return;                                            // (a NaN fails its comparison: the point is dropped)
  const float r = nx * dx + ny * dy + nz * dz;
  const float ar = fabsf(r);
  const float w = ar <= a.huber ? 1.0f : a.huber / ar;
  const double J[6] = {nx, ny, nz, P.y * nz - P.z * ny, P.z * nx - P.x * nz, P.x * ny - P.y * nx};   // [n, p' x n]
  const double rd = r, wd = w;
  int m = 0;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    const double wj = wd * J[i];
#pragma unroll
    for (int j = i; j < 6; ++j, ++m) acc[m] = fma(wj, J[j], acc[m]);
    acc[ICP_A + i] = fma(wj, rd, acc[ICP_A + i]);
  }
  acc[ICP_E] = fma(wd * rd, rd, acc[ICP_E]);
  ++cnt;
}

// A xi = -b by a 6x6 Cholesky; s = the 21 entries of A's upper triangle by rows, then b.  false: a pivot that is not positive and
// finite, or a step that is not finite.
__device__ bool icp_solve(const double* s, double (&xi)[6]) {
  double A[6][6], L[6][6];
  int m = 0;
  for (int i = 0; i < 6; ++i)
    for (int j = i; j < 6; ++j) A[i][j] = A[j][i] = s[m++];
  for (int j = 0; j < 6; ++j) {
    double d = A[j][j];
    for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k];
    if (!(d > 0.0 && d < (double)INFINITY)) return false;
    const double l = sqrt(d);
    L[j][j] = l;
    for (int i = j + 1; i < 6; ++i) {
      double v = A[i][j];
      for (int k = 0; k < j; ++k) v -= L[i][k] * L[j][k];
      L[i][j] = v / l;
    }
  }
  double y[6];
  for (int i = 0; i < 6; ++i) {
    double v = -s[ICP_A + i];
    for (int k = 0; k < i; ++k) v -= L[i][k] * y[k];
    y[i] = v / L[i][i];
  }
  for (int i = 5; i >= 0; --i) {
    double v = y[i];
    for (int k = i + 1; k < 6; ++k) v -= L[k][i] * xi[k];
    xi[i] = v / L[i][i];
  }
  for (int i = 0; i < 6; ++i)
    if (!(fabs(xi[i]) < (double)INFINITY)) return false;
  return true;
}

// Tn = exp(xi) T, xi = (v, omega); T = 9 rotation entries by rows, then the translation.  false when Tn is not finite (|omega|^2 can
// overflow for a finite but huge step out of a nearly singular system): the caller keeps T.
__device__ bool icp_update(const double* T, const double (&xi)[6], double (&Tn)[12]) {
  const double wx = xi[3], wy = xi[4], wz = xi[5];
  const double th2 = wx * wx + wy * wy + wz * wz, th = sqrt(th2);
  double a, b, c;                       // sin th / th, (1 - cos th) / th^2, (th - sin th) / th^3
  if (th < 1e-4) {
    a = 1.0 - th2 / 6.0;
    b = 0.5 - th2 / 24.0;
    c = 1.0 / 6.0 - th2 / 120.0;
  } else {
    const double s = sin(th), co = cos(th);
    a = s / th;
    b = (1.0 - co) / th2;
    c = (th - s) / (th2 * th);
  }
  const double K[9] = {0, -wz, wy, wz, 0, -wx, -wy, wx, 0};
  double K2[9], dR[9], V[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) K2[3 * i + j] = K[3 * i] * K[j] + K[3 * i + 1] * K[3 + j] + K[3 * i + 2] * K[6 + j];
  for (int i = 0; i < 9; ++i) {
    const double id = (i % 4 == 0) ? 1.0 : 0.0;
    dR[i] = id + a * K[i] + b * K2[i];
    V[i] = id + b * K[i] + c * K2[i];
  }
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) Tn[3 * i + j] = dR[3 * i] * T[j] + dR[3 * i + 1] * T[3 + j] + dR[3 * i + 2] * T[6 + j];
    Tn[9 + i] = dR[3 * i] * T[9] + dR[3 * i + 1] * T[10] + dR[3 * i + 2] * T[11] + V[3 * i] * xi[0] + V[3 * i + 1] * xi[1] +
                V[3 * i + 2] * xi[2];
  }
  for (int i = 0; i < 12; ++i)
    if (!(fabs(Tn[i]) < (double)INFINITY)) return false;
  return true;
}

// VEC: H * W is a multiple of 4 and the three maps are 16-byte aligned (every scan's slice then is).  The scalar form walks the same
// groups in the same order: the same sums.
template <bool VEC>
__global__ __launch_bounds__(ICP_THREADS) void icp_register_kernel(const IcpArgs a) {
  __shared__ double s_T[12];
  __shared__ double s_part[ICP_WAVES][ICP_SUMS];
  __shared__ double s_sum[ICP_SUMS];
  __shared__ int s_stop;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t pair = blockIdx.x;
  const double* T0 = a.init_pose + 16 * pair;
  const int si = a.src_idx[pair], ti = a.tgt_idx[pair];
  if (si < 0 || si >= a.n_scans || ti < 0 || ti >= a.n_scans) {      // reads no map
    if (tid < 16) a.pose[16 * pair + tid] = T0[tid];
    if (tid < 8) a.stats[8 * pair + tid] = tid == 0 ? 2.0 : 0.0;
    if (a.system && tid < 28) a.system[28 * pair + tid] = 0.0;
    return;
  }
  const int HW = a.H * a.W;
  const int groups = (int)(((int64_t)HW + 3) >> 2);      // H * W may be 2^31 - 1: group and pixel offsets in 64 bits
  const float* __restrict__ rs = a.range + (size_t)si * HW;
  const float* __restrict__ vs = a.vertex + (size_t)si * HW * 4;
  const float* __restrict__ ns = a.normal + (size_t)si * HW * 3;
  const float* __restrict__ rt = a.range + (size_t)ti * HW;
  const float* __restrict__ vt = a.vertex + (size_t)ti * HW * 4;
  const float* __restrict__ nt = a.normal + (size_t)ti * HW * 3;

  if (tid < 12) s_T[tid] = tid < 9 ? T0[(tid / 3) * 4 + tid % 3] : T0[(tid - 9) * 4 + 3];
  if (tid == 0) s_stop = 0;
  __syncthreads();

  // thread 0 only
  int status = 0, solved = 0;
  double step_v = 0.0, step_w = 0.0, last_e = 0.0, last_count = 0.0, last_valid = 0.0;

  for (int pass = 0; pass <= a.iterations; ++pass) {
    IcpPose T;
#pragma unroll
    for (int i = 0; i < 9; ++i) T.r[i] = (float)s_T[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) T.t[i] = (float)s_T[9 + i];

    double acc[ICP_ACC];
#pragma unroll
    for (int i = 0; i < ICP_ACC; ++i) acc[i] = 0.0;
    int cnt = 0, valid = 0;

    for (int g = tid; g < groups; g += ICP_THREADS) {
      const int64_t p0 = 4 * (int64_t)g;
      float rg[4], pv[16], nv[12];
      if (VEC) {      // eight 16-byte loads in flight, whether or not the group has a valid pixel
        const f32x4 v = reinterpret_cast<const f32x4*>(rs)[g];
        rg[0] = v.x, rg[1] = v.y, rg[2] = v.z, rg[3] = v.w;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const f32x4 q = reinterpret_cast<const f32x4*>(vs)[p0 + k];
          pv[4 * k] = q.x, pv[4 * k + 1] = q.y, pv[4 * k + 2] = q.z, pv[4 * k + 3] = q.w;
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const f32x4 q = reinterpret_cast<const f32x4*>(ns)[3 * (int64_t)g + k];
          nv[4 * k] = q.x, nv[4 * k + 1] = q.y, nv[4 * k + 2] = q.z, nv[4 * k + 3] = q.w;
        }
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const bool in = p0 + k < HW;
          rg[k] = in ? rs[p0 + k] : 0.0f;
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            pv[4 * k + c] = in ? vs[(p0 + k) * 4 + c] : 0.0f;
            nv[3 * k + c] = in ? ns[(p0 + k) * 3 + c] : -1.0f;
          }
        }
      }
      IcpPoint P[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const bool v = rg[k] > 0.0f;
        valid += v ? 1 : 0;
        P[k] = icp_project(a, T, v, pv[4 * k], pv[4 * k + 1], pv[4 * k + 2], nv[3 * k], nv[3 * k + 1], nv[3 * k + 2]);
      }
      // 2. the four points' target data: twenty loads issued before any is used
      float q[4][3], n[4][3], rq[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const size_t pix = (size_t)P[k].pix;
        rq[k] = rt[pix];
        if (VEC) {
          const f32x4 v = reinterpret_cast<const f32x4*>(vt)[pix];
          q[k][0] = v.x, q[k][1] = v.y, q[k][2] = v.z;
        } else {
          q[k][0] = vt[4 * pix], q[k][1] = vt[4 * pix + 1], q[k][2] = vt[4 * pix + 2];
        }
        n[k][0] = nt[3 * pix], n[k][1] = nt[3 * pix + 1], n[k][2] = nt[3 * pix + 2];
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) icp_accumulate(a, P[k], q[k][0], q[k][1], q[k][2], n[k][0], n[k][1], n[k][2], rq[k], acc, cnt);
    }

    // fixed tree: the wave, then the 8 waves in order
    double red[ICP_SUMS];
#pragma unroll
    for (int i = 0; i < ICP_ACC; ++i) red[i] = acc[i];
    red[ICP_COUNT] = (double)cnt;
    red[ICP_VALID] = (double)valid;
#pragma unroll
    for (int i = 0; i < ICP_SUMS; ++i) {
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) red[i] += __shfl_down(red[i], off, 64);
      if (lane == 0) s_part[wave][i] = red[i];
    }
    __syncthreads();
    if (tid < ICP_SUMS) {
      double s = 0.0;
#pragma unroll
      for (int w = 0; w < ICP_WAVES; ++w) s += s_part[w][tid];
      s_sum[tid] = s;
    }
    __syncthreads();

    if (pass == 0 && a.system && tid < 28) a.system[28 * pair + tid] = tid < ICP_E ? s_sum[tid] : s_sum[ICP_COUNT];
    if (tid == 0) {
      last_e = s_sum[ICP_E];
      last_count = s_sum[ICP_COUNT];
      last_valid = s_sum[ICP_VALID];
      bool stop = pass == a.iterations;
      if (last_count < (double)a.min_inliers) {
        status = 1;
        stop = true;
      } else if (!stop) {
        double xi[6], Tn[12];
        if (icp_solve(s_sum, xi) && icp_update(s_T, xi, Tn)) {
          for (int i = 0; i < 12; ++i) s_T[i] = Tn[i];
          ++solved;
          step_v = sqrt(xi[0] * xi[0] + xi[1] * xi[1] + xi[2] * xi[2]);
          step_w = sqrt(xi[3] * xi[3] + xi[4] * xi[4] + xi[5] * xi[5]);
        } else {
          status = 1;
          stop = true;
        }
      }
      s_stop = stop ? 1 : 0;
    }
    __syncthreads();
    if (s_stop) break;
  }

  if (tid == 0) {
    double* P = a.pose + 16 * pair;
    if (solved == 0) {
      for (int i = 0; i < 16; ++i) P[i] = T0[i];          // T0 bit for bit, its last row included
    } else {
      for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) P[4 * i + j] = s_T[3 * i + j];
        P[4 * i + 3] = s_T[9 + i];
      }
      P[12] = P[13] = P[14] = 0.0;
      P[15] = 1.0;
    }
    double* S = a.stats + 8 * pair;
    S[0] = (double)status;
    S[1] = (double)solved;
    S[2] = last_count;
    S[3] = last_valid;
    S[4] = last_count > 0.0 ? sqrt(fmax(last_e, 0.0) / last_count) : 0.0;
    S[5] = step_v;
    S[6] = step_w;
    S[7] = 0.0;
  }
}

}  // namespace

int ovn_icp_register_forward(const float* vertex, const float* normal, const float* range, int n_scans, int H, int W,
                             double fov_up_deg, double fov_down_deg, double max_range, const int32_t* src_idx, const int32_t* tgt_idx,
                             int n_pairs, const double* init_pose, int iterations, double max_dist, double cos_min, double huber,
                             int min_inliers, double* pose, double* stats, double* system, hipStream_t stream) {
  if (n_pairs == 0) return OVN_OK;
  const double pi = 3.14159265358979323846;
  const double up = fov_up_deg / 180.0 * pi, down = fov_down_deg / 180.0 * pi;
  IcpArgs a;
  a.vertex = vertex, a.normal = normal, a.range = range;
  a.n_scans = n_scans, a.H = H, a.W = W;
  a.fov_down_abs = (float)fabs(down);
  a.inv_fov = (float)(1.0 / (fabs(down) + fabs(up)));
  a.max_range = (float)max_range;
  a.src_idx = src_idx, a.tgt_idx = tgt_idx, a.init_pose = init_pose;
  a.iterations = iterations;
  a.max_dist2 = (float)(max_dist * max_dist), a.cos_min = (float)cos_min, a.huber = (float)huber;
  a.min_inliers = min_inliers;
  a.pose = pose, a.stats = stats, a.system = system;
  const uintptr_t bases = reinterpret_cast<uintptr_t>(vertex) | reinterpret_cast<uintptr_t>(normal) | reinterpret_cast<uintptr_t>(range);
  const bool vec = ((int64_t)H * W) % 4 == 0 && (bases & 15) == 0;
  if (vec)
    hipLaunchKernelGGL(icp_register_kernel<true>, dim3((unsigned)n_pairs), dim3(ICP_THREADS), 0, stream, a);
  else
    hipLaunchKernelGGL(icp_register_kernel<false>, dim3((unsigned)n_pairs), dim3(ICP_THREADS), 0, stream, a);
  OVN_HIP_CHECK(hipGetLastError());
  return OVN_OK;
}
