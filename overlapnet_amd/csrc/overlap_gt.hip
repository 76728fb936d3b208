// Ground-truth overlap between a frame and N reference scans for gfx950 (the label producer next to the hot path).
//
// Reference (src/utils/com_overlap_yaw.py:28-46): every reference scan is moved into the current frame,
//     p_world = pose_ref . p,   p_cur = inv(pose_cur) . p_world            (two float64 matrix products, :37-39)
// range-projected IN FLOAT64 (range_projection on load_vertex's float64 points, utils.py:59-134,217-230), and
//     overlap = #{ pixels : ref_range > 0 and |ref_range - cur_range| < 1 } / #{ cur_range > 0 }.
// Only the range image is needed, so "nearest point wins" is a 32-bit atomicMin over the float32 bits of the depth
// (the image is float32, utils.py:120-121; positive floats order like their bit patterns).  HBM-bound: 16 B per point in,
// one atomic per kept point; one workgroup row per scan so that ragged scans need no host-side padding.
// Compiled with -ffp-contract=off: the fused multiply-adds below are explicit.
#include <math.h>

#include "ovn_internal.h"

namespace {

constexpr unsigned EMPTY = 0xFFFFFFFFu;

__global__ __launch_bounds__(256) void gt_fill_kernel(unsigned* __restrict__ img, long long n) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
    img[i] = EMPTY;
}

// dot of a pose row with (x, y, z, 1) the way a BLAS dgemm micro-kernel accumulates it: k = 0..3, fused
__device__ __forceinline__ double row_dot(const double* __restrict__ r, double x, double y, double z) {
  double acc = r[0] * x;
  acc = fma(r[1], y, acc);
  acc = fma(r[2], z, acc);
  acc = fma(r[3], 1.0, acc);
  return acc;
}

// One point of scan s seen from the current frame: p' = inv_cur_pose . (ref_pose . p) as two sequential float64 products
// (com_overlap_yaw.py:37-39), then range_projection's pixel and float32 depth (utils.py:75-121).  false = the range filter drops
// the point.  The ONLY copy of this arithmetic: gt_scatter_kernel and gt_pair_kernel both call it, so a pair's pixel and depth
// bits are the range image's by construction.
__device__ __forceinline__ bool gt_project_point(const f32x4 p, const double* __restrict__ ref_pose,
                                                 const double* __restrict__ inv_cur_pose, int H, int W, double fov_down_abs,
                                                 double fov, double max_range, int& pix, float& depth32) {
  double x = (double)p[0], y = (double)p[1], z = (double)p[2];
  if (ref_pose) {
    const double wx = row_dot(ref_pose, x, y, z), wy = row_dot(ref_pose + 4, x, y, z), wz = row_dot(ref_pose + 8, x, y, z);
    x = wx;
    y = wy;
    z = wz;
  }
  if (inv_cur_pose) {
    const double cx = row_dot(inv_cur_pose, x, y, z), cy = row_dot(inv_cur_pose + 4, x, y, z),
                 cz = row_dot(inv_cur_pose + 8, x, y, z);
    x = cx;
    y = cy;
    z = cz;
  }
  const double depth = sqrt((x * x + y * y) + z * z);
  if (!(depth > 0.0 && depth < max_range)) return false;
  const double yaw = -atan2(y, x);
  const double pitch = asin(z / depth);
  double px = 0.5 * (yaw / 3.141592653589793 + 1.0);
  double py = 1.0 - (pitch + fov_down_abs) / fov;
  px = floor(px * (double)W);
  py = floor(py * (double)H);
  px = fmax(0.0, fmin((double)(W - 1), px));
  py = fmax(0.0, fmin((double)(H - 1), py));
  pix = (int)py * W + (int)px;
  depth32 = (float)depth;
  return true;
}

__global__ __launch_bounds__(256) void gt_scatter_kernel(const float* __restrict__ points, const int64_t* __restrict__ offsets,
                                                         const double* __restrict__ ref_poses,
                                                         const double* __restrict__ inv_cur_pose, int H, int W, double fov_down_abs,
                                                         double fov, double max_range, unsigned* __restrict__ img) {
  const int s = blockIdx.y;
  const long long beg = offsets[s], end = offsets[s + 1];
  const long long i = beg + (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= end) return;
  const f32x4 p = *reinterpret_cast<const f32x4*>(points + 4 * i);
  int pix;
  float d;
  if (!gt_project_point(p, ref_poses ? ref_poses + 16 * (long long)s : nullptr, inv_cur_pose, H, W, fov_down_abs, fov, max_range,
                        pix, d))
    return;
  atomicMin(img + (long long)s * H * W + pix, __float_as_uint(d));
}

// Overlap count of one (frame, reference scan) pair per workgroup WITHOUT the pair's range image.  A pixel counts in
// gt_count_kernel iff the nearest projected depth m has m > 0 and |m - c| < 1 (c = the frame's own range there).  Two flags per
// pixel, set while the points stream by (d = a point's float32 depth), decide the same thing:
//   hit:     d > 0 and |d - c| < 1
//   blocked: d <= 0 (a depth that rounds to 0f wins the minimum and is not > 0), or d < c and not |d - c| < 1
// count = #{hit and not blocked}: float32 subtraction is monotone, so a point nearer than a hit is itself a hit or blocks, and
// a point beyond c that is no hit lies beyond every hit.  The planes live in LDS (2 x ceil(HW/32) words, 14,400 B
// at 64 x 900): no global image, no fill / finish / count pass, no global atomic.
// pair = pair_base + blockIdx.x; frame_fastest picks which of the two indices varies between neighbouring workgroups.
__global__ __launch_bounds__(256) void gt_pair_kernel(const float* __restrict__ points, const int64_t* __restrict__ offsets,
                                                      int n_scans, const double* __restrict__ poses,
                                                      const double* __restrict__ inv_poses, const float* __restrict__ cur_ranges,
                                                      const int32_t* __restrict__ frame_idx, int n_frames,
                                                      const int32_t* __restrict__ ref_idx, int n_refs, long long pair_base,
                                                      int frame_fastest, int H, int W, double fov_down_abs, double fov,
                                                      double max_range, int32_t* __restrict__ counts) {
  extern __shared__ unsigned planes[];      // 2 * words, at least 4: the wave partials reuse it, so 64 KB of planes still launch
  const int npix = H * W, words = (npix + 31) >> 5;
  unsigned* hit = planes;
  unsigned* blocked = planes + words;
  const long long pair = pair_base + blockIdx.x;
  const int fi = frame_fastest ? (int)(pair % n_frames) : (int)(pair / n_refs);
  const int ri = frame_fastest ? (int)(pair / n_frames) : (int)(pair % n_refs);
  const int f = frame_idx ? frame_idx[fi] : fi, r = ref_idx ? ref_idx[ri] : ri;
  int32_t* out = counts + (long long)fi * n_refs + ri;
  if (f < 0 || f >= n_scans || r < 0 || r >= n_scans) {      // an index outside the sequence: no read, the pair reports -1
    if (threadIdx.x == 0) *out = -1;
    return;
  }
  for (int w = threadIdx.x; w < 2 * words; w += 256) planes[w] = 0u;
  __syncthreads();
  const double* P = poses + 16 * (long long)r;
  const double* Inv = inv_poses + 16 * (long long)f;
  const float* cur = cur_ranges + (long long)f * npix;
  const long long end = offsets[r + 1];
  for (long long i = offsets[r] + threadIdx.x; i < end; i += 256) {
    const f32x4 p = *reinterpret_cast<const f32x4*>(points + 4 * i);
    int pix;
    float d;
    if (!gt_project_point(p, P, Inv, H, W, fov_down_abs, fov, max_range, pix, d)) continue;
    const float c = cur[pix];
    const bool near = fabsf(d - c) < 1.0f;
    const unsigned bit = 1u << (pix & 31);
    if (d > 0.0f && near) atomicOr(hit + (pix >> 5), bit);
    if (d <= 0.0f || (d < c && !near)) atomicOr(blocked + (pix >> 5), bit);
  }
  __syncthreads();
  int c = 0;
  for (int w = threadIdx.x; w < words; w += 256) c += __popc(hit[w] & ~blocked[w]);     // bits beyond H*W are never set
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off, 64);
  __syncthreads();                          // every plane word is read: the planes may take the four wave partials
  if ((threadIdx.x & 63) == 0) planes[threadIdx.x >> 6] = (unsigned)c;
  __syncthreads();
  if (threadIdx.x == 0) *out = (int32_t)(planes[0] + planes[1] + planes[2] + planes[3]);
}

// uint image -> float range image in place (-1 = empty)
__global__ __launch_bounds__(256) void gt_finish_kernel(unsigned* __restrict__ img, long long n) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const unsigned v = img[i];
    if (v == EMPTY) img[i] = __float_as_uint(-1.0f);
  }
}

// counts[s] = #{ref > 0 and |ref - cur| < 1}; counts[n] = #{cur > 0} (block n)
__global__ __launch_bounds__(256) void gt_count_kernel(const float* __restrict__ ref, const float* __restrict__ cur, int npix,
                                                       int n, int32_t* __restrict__ counts) {
  __shared__ int part[4];
  const int s = blockIdx.x;
  int c = 0;
  if (s < n) {
    const float* r = ref + (long long)s * npix;
    // unsigned counters: the last i + 256 passes 2^31 - 1 when npix is within 256 of it (npix <= 2^31 - 1 always)
    for (uint32_t i = threadIdx.x; i < (uint32_t)npix; i += 256) {
      const float v = r[i];
      if (v > 0.0f && fabsf(v - cur[i]) < 1.0f) ++c;
    }
  } else {
    for (uint32_t i = threadIdx.x; i < (uint32_t)npix; i += 256)
      if (cur[i] > 0.0f) ++c;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) counts[s] = part[0] + part[1] + part[2] + part[3];
}

}  // namespace

int ovn_gt_range_forward(const float* points, const int64_t* offsets, int n_scans, long long max_points, const double* ref_poses,
                         const double* inv_cur_pose, int H, int W, double fov_up_deg, double fov_down_deg, double max_range,
                         float* range_out, hipStream_t stream) {
  const long long total = (long long)n_scans * H * W;
  if (total == 0) return OVN_OK;
  unsigned* img = reinterpret_cast<unsigned*>(range_out);
  hipLaunchKernelGGL(gt_fill_kernel, dim3(1024), dim3(256), 0, stream, img, total);
  if (max_points > 0) {
    const double up = fov_up_deg / 180.0 * 3.141592653589793, down = fov_down_deg / 180.0 * 3.141592653589793;
    const double fov = fabs(down) + fabs(up);
    dim3 grid((unsigned)((max_points + 255) / 256), (unsigned)n_scans);
    hipLaunchKernelGGL(gt_scatter_kernel, grid, dim3(256), 0, stream, points, offsets, ref_poses, inv_cur_pose, H, W, fabs(down),
                       fov, max_range, img);
  }
  hipLaunchKernelGGL(gt_finish_kernel, dim3(1024), dim3(256), 0, stream, img, total);
  OVN_HIP_CHECK(hipGetLastError());
  return OVN_OK;
}

int ovn_gt_count_forward(const float* ref_ranges, const float* cur_range, int n, int npix, int32_t* counts, hipStream_t stream) {
  hipLaunchKernelGGL(gt_count_kernel, dim3(n + 1), dim3(256), 0, stream, ref_ranges, cur_range, npix, n, counts);
  OVN_HIP_CHECK(hipGetLastError());
  return OVN_OK;
}

int ovn_gt_pair_forward(const float* points, const int64_t* offsets, int n_scans, const double* poses, const double* inv_poses,
                        const float* cur_ranges, const int32_t* frame_idx, int n_frames, const int32_t* ref_idx, int n_refs, int H,
                        int W, double fov_up_deg, double fov_down_deg, double max_range, int frame_fastest, int32_t* counts,
                        hipStream_t stream) {
  const long long pairs = (long long)n_frames * n_refs;
  const int words = (H * W + 31) >> 5;
  const size_t lds = (size_t)(2 * words > 4 ? 2 * words : 4) * sizeof(unsigned);
  const double up = fov_up_deg / 180.0 * 3.141592653589793, down = fov_down_deg / 180.0 * 3.141592653589793;
  const double fov = fabs(down) + fabs(up);
  // a launch holds at most 2^32 - 1 threads: 2^23 workgroups of 256 per launch, the pair index carried in pair_base
  constexpr long long kPairsPerLaunch = 1ll << 23;
  for (long long base = 0; base < pairs; base += kPairsPerLaunch) {
    const long long n = pairs - base < kPairsPerLaunch ? pairs - base : kPairsPerLaunch;
    hipLaunchKernelGGL(gt_pair_kernel, dim3((unsigned)n), dim3(256), lds, stream, points, offsets, n_scans, poses, inv_poses,
                       cur_ranges, frame_idx, n_frames, ref_idx, n_refs, base, frame_fastest, H, W, fabs(down), fov, max_range,
                       counts);
  }
  OVN_HIP_CHECK(hipGetLastError());
  return OVN_OK;
}
