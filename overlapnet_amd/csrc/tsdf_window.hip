// The rolling TSDF window moves: the slots whose samples leave are cleared for the samples that enter (ovn_tsdf_window_shift; DESIGN.md
// section 36).  The window's other three calls -- integrate, ray cast, triangles -- are the RING instantiations of the dense kernels in
// tsdf.hip and tsdf_raycast.hip; the addressing they share is OvnRing in ovn_internal.h.
//
// A window (nx,ny,nz) at `base` holds sample I of an axis in slot I mod n.  Moving the base by d on an axis makes min(|d|, n) samples of
// that axis enter; they take the slots of the samples that leave: a slab of that many slots, whole in the other two axes.  One launch per
// moved axis over its slab alone, one lane per slot, x fastest; a slot in two slabs gets the same two words twice.  No LDS, no atomics.
#include "ovn_internal.h"

namespace {

struct ClearArgs {
  float* tsdf;
  float* weight;
  long long total;      // count[0] count[1] count[2]
  int n[3];
  int start[3];         // the slab: slots start .. start + count - 1 (mod n) on every axis
  int count[3];
};

__global__ __launch_bounds__(256) void tsdf_window_clear_kernel(ClearArgs a) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= a.total) return;
  const long long row = t / a.count[0];
  int x = a.start[0] + (int)(t - row * a.count[0]);
  const int w = (int)(row / a.count[1]);
  int y = a.start[1] + (int)(row - (long long)w * a.count[1]);
  int z = a.start[2] + w;
  if (x >= a.n[0]) x -= a.n[0];                  // start < n and count <= n: one subtraction lands in 0 .. n - 1
  if (y >= a.n[1]) y -= a.n[1];
  if (z >= a.n[2]) z -= a.n[2];
  const long long idx = ((long long)z * a.n[1] + y) * a.n[0] + x;
  a.tsdf[idx] = 1.0f;
  a.weight[idx] = 0.0f;
}

int floor_mod(int v, int n) {
  const int m = v % n;
  return m < 0 ? m + n : m;
}

}  // namespace

int ovn_tsdf_window_shift_forward(float* tsdf, float* weight, int nx, int ny, int nz, const int* old_base, const int* new_base,
                                  hipStream_t stream) {
  const int n[3] = {nx, ny, nz};
  long long d[3];
  bool all = false;
  for (int x = 0; x < 3; ++x) {
    d[x] = (long long)new_base[x] - old_base[x];
    all = all || d[x] >= n[x] || -d[x] >= n[x];
  }
  for (int x = 0; x < 3; ++x) {
    if (!all && d[x] == 0) continue;
    ClearArgs a;
    a.tsdf = tsdf;
    a.weight = weight;
    for (int y = 0; y < 3; ++y) {
      a.n[y] = n[y];
      a.start[y] = 0;
      a.count[y] = n[y];
    }
    if (!all) {
      // d > 0: samples old + n .. new + n - 1 enter, the first in the slot of old_base; d < 0: samples new .. old - 1, from new's slot
      a.start[x] = floor_mod(d[x] > 0 ? old_base[x] : new_base[x], n[x]);
      a.count[x] = (int)(d[x] > 0 ? d[x] : -d[x]);
    }
    a.total = (long long)a.count[0] * a.count[1] * a.count[2];      // <= nx ny nz < 2^31
    hipLaunchKernelGGL(tsdf_window_clear_kernel, dim3((unsigned)((a.total + 255) / 256)), dim3(256), 0, stream, a);
    OVN_HIP_CHECK(hipGetLastError());
    if (all) break;                              // a whole window or more: the one launch covered every slot
  }
  return OVN_OK;
}
