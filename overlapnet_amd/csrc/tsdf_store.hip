// Whole 8 x 8 x 8 bricks between the rolling TSDF window and a pool of brick slots (ovn_tsdf_window_brick_flags / _page_out / _page_in,
// include/ovn_hip_tsdf_store.h): what leaves the window is kept, and put back when the window returns.
//
// A window's dimensions and base are multiples of 8, so it holds whole lattice bricks, a brick's eight slots on every axis are
// consecutive (the seam is a multiple of 8 too) and its eight x samples are one aligned 32-byte run of a row.  A brick is therefore
// 64 rows x 2 arrays x 2 float4 = 256 16-byte pieces, and piece p of a brick is float4 p of its 4 KB pool slot:
//   p = array * 128 + (z * 8 + y) * 2 + half        array 0 = tsdf, 1 = weight
// Paging: one workgroup of 256 threads per brick, thread p moves piece p -- one 16-byte load and one 16-byte store.  The pool side is
// 4 KB contiguous (each wave 1 KB, fully coalesced); the ring side is 32-byte runs, which is what the layout of a dense volume leaves.
// Flags: one wave per brick, lane l reads pieces l, l + 64, l + 128, l + 192 and a ballot joins the comparisons.  The three ring slots
// of a brick are computed once per brick with ovn_ring_slot.  No LDS, no atomics, no scratch.
#include "ovn_internal.h"
#include "../../include/ovn_hip_tsdf_store.h"

namespace {

constexpr int STORE_THREADS = 256;
constexpr int STORE_MAX_INDEX = 1 << 20;         // WINDOW_MAX_INDEX of ovn_api.hip
constexpr int BRICK_PIECES = OVN_TSDF_BRICK_WORDS / 4;

struct StoreWindow {
  float* tsdf;
  float* weight;
  int n[3];
  OvnRing ring;
};

// the first float4 of piece p of brick (b[0], b[1], b[2]) in ring storage, given the ring slots s[3] of the brick's first sample
__device__ __forceinline__ long long ring_piece(const StoreWindow& w, const int* s, int p, int* array) {
  *array = p >> 7;
  const int r = p & 127;
  const int row = r >> 1, half = r & 1;
  const int z = s[2] + (row >> 3), y = s[1] + (row & 7), x = s[0] + half * 4;
  return (((long long)z * w.n[1] + y) * w.n[0] + x) >> 2;          // x is a multiple of 4 and nx of 8: a whole float4 index
}

// the brick's ring slots; false for a brick outside the window
__device__ __forceinline__ bool brick_slots(const StoreWindow& w, int bi, int bj, int bk, int* s) {
  const int b[3] = {bi, bj, bk};
  bool inside = true;
  for (int a = 0; a < 3; ++a) {
    const long long I = (long long)b[a] * 8;
    inside = inside && I >= w.ring.base[a] && I + 8 <= (long long)w.ring.base[a] + w.n[a];
  }
  if (!inside) return false;
  for (int a = 0; a < 3; ++a) s[a] = ovn_ring_slot(b[a] * 8, w.ring.base[a], w.ring.slot0[a], w.n[a]);
  return true;
}

template <bool OUT>
__global__ __launch_bounds__(STORE_THREADS) void tsdf_store_page_kernel(StoreWindow w, const int* __restrict__ bricks,
                                                                        const int* __restrict__ slots, float4* __restrict__ pool) {
  const long long i = blockIdx.x;
  const int slot = slots[i];
  int s[3];
  if (slot < 0 || !brick_slots(w, bricks[3 * i], bricks[3 * i + 1], bricks[3 * i + 2], s)) return;      // uniform over the workgroup
  const int p = threadIdx.x;
  int array;
  const long long r = ring_piece(w, s, p, &array);
  float4* ring = reinterpret_cast<float4*>(array ? w.weight : w.tsdf) + r;
  float4* home = pool + (long long)slot * BRICK_PIECES + p;
  if (OUT) *home = *ring; else *ring = *home;
}

struct FlagArgs {
  int lo[3];
  int count[3];
  long long total;
};

__global__ __launch_bounds__(STORE_THREADS) void tsdf_store_flags_kernel(StoreWindow w, FlagArgs f, unsigned char* __restrict__ flags) {
  const long long i = (long long)blockIdx.x * (STORE_THREADS / 64) + (threadIdx.x >> 6);        // one wave per brick
  if (i >= f.total) return;
  const int lane = threadIdx.x & 63;
  const long long row = i / f.count[0];
  const int bx = f.lo[0] + (int)(i - row * f.count[0]);
  const int bz = f.lo[2] + (int)(row / f.count[1]);
  const int by = f.lo[1] + (int)(row - (row / f.count[1]) * f.count[1]);
  int s[3];
  bool differs = false;
  if (brick_slots(w, bx, by, bz, s)) {            // the host checked the box: always true
    for (int k = 0; k < 4; ++k) {
      int array;
      const long long r = ring_piece(w, s, k * 64 + lane, &array);
      const uint4 v = *(reinterpret_cast<const uint4*>(array ? w.weight : w.tsdf) + r);
      const unsigned fresh = array ? 0u : 0x3f800000u;
      differs = differs || v.x != fresh || v.y != fresh || v.z != fresh || v.w != fresh;
    }
  }
  const unsigned long long any = __ballot(differs);
  if (lane == 0) flags[i] = any != 0ull ? 1 : 0;
}

bool store_window_ok(int nx, int ny, int nz, const int* base, StoreWindow* w) {
  const int n[3] = {nx, ny, nz};
  if (!base) return false;
  for (int a = 0; a < 3; ++a) {
    if (n[a] < 16 || n[a] % 8 != 0 || base[a] % 8 != 0) return false;
    if (base[a] < -STORE_MAX_INDEX || (int64_t)base[a] + n[a] - 1 > STORE_MAX_INDEX) return false;
    const int m = base[a] % n[a];
    w->n[a] = n[a];
    w->ring.base[a] = base[a];
    w->ring.slot0[a] = m < 0 ? m + n[a] : m;
  }
  return (int64_t)nx * ny * nz <= 2147483647ll;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

#define OVN_STORE_WINDOW(fn)                                                                                                       \
  OVN_REQUIRE(ctx != nullptr, OVN_ERR_ARG, fn ": ctx is NULL");                                                                    \
  OVN_REQUIRE(tsdf_dev && weight_dev && base, OVN_ERR_ARG, fn ": NULL volume buffer or base");                                     \
  StoreWindow w;                                                                                                                   \
  OVN_REQUIRE(store_window_ok(nx, ny, nz, base, &w), OVN_ERR_ARG,                                                                  \
              fn ": window %d x %d x %d at base (%d, %d, %d): dimensions and base must be multiples of 8, dimensions >= 16, at "   \
                 "most 2^31 - 1 samples, every index within 2^20",                                                                \
              nx, ny, nz, base[0], base[1], base[2]);                                                                              \
  OVN_REQUIRE(aligned16(tsdf_dev) && aligned16(weight_dev), OVN_ERR_ARG, fn ": tsdf and weight must be 16-byte aligned");          \
  w.tsdf = const_cast<float*>(tsdf_dev);                                                                                           \
  w.weight = const_cast<float*>(weight_dev)

template <bool OUT>
int page(const char* fn, ovn_ctx* ctx, void* stream, const StoreWindow& w, int n, const int32_t* bricks_dev, const int32_t* slots_dev,
         const float* pool_dev) {
  OVN_REQUIRE(bricks_dev && slots_dev && pool_dev, OVN_ERR_ARG, "%s: NULL bricks, slots or pool", fn);
  OVN_REQUIRE(aligned16(pool_dev), OVN_ERR_ARG, "%s: the pool must be 16-byte aligned", fn);
  OVN_ON_DEVICE(ctx->device);
  hipLaunchKernelGGL(tsdf_store_page_kernel<OUT>, dim3((unsigned)n), dim3(STORE_THREADS), 0, (hipStream_t)stream, w, bricks_dev,
                     slots_dev, reinterpret_cast<float4*>(const_cast<float*>(pool_dev)));
  OVN_HIP_CHECK(hipGetLastError());
  return OVN_OK;
}

}  // namespace

extern "C" int ovn_tsdf_window_brick_flags(ovn_ctx* ctx, void* stream, const float* tsdf_dev, const float* weight_dev, int nx, int ny,
                                           int nz, const int32_t* base, const int32_t* box_lo, const int32_t* box_hi,
                                           uint8_t* flags_dev) {
  OVN_STORE_WINDOW("ovn_tsdf_window_brick_flags");
  OVN_REQUIRE(box_lo && box_hi, OVN_ERR_ARG, "ovn_tsdf_window_brick_flags: NULL box");
  FlagArgs f;
  f.total = 1;
  for (int a = 0; a < 3; ++a) {
    OVN_REQUIRE(box_lo[a] <= box_hi[a] && (int64_t)box_lo[a] * 8 >= base[a] && (int64_t)box_hi[a] * 8 <= (int64_t)base[a] + w.n[a],
                OVN_ERR_ARG, "ovn_tsdf_window_brick_flags: bricks %d .. %d of axis %d lie outside the window's bricks %d .. %d", box_lo[a],
                box_hi[a] - 1, a, base[a] / 8, (base[a] + w.n[a]) / 8 - 1);
    f.lo[a] = box_lo[a];
    f.count[a] = box_hi[a] - box_lo[a];
    f.total *= f.count[a];                      // <= nx ny nz / 512
  }
  if (f.total == 0) return OVN_OK;
  OVN_REQUIRE(flags_dev != nullptr, OVN_ERR_ARG, "ovn_tsdf_window_brick_flags: flags is NULL");
  OVN_ON_DEVICE(ctx->device);
  const long long per = STORE_THREADS / 64;
  hipLaunchKernelGGL(tsdf_store_flags_kernel, dim3((unsigned)((f.total + per - 1) / per)), dim3(STORE_THREADS), 0, (hipStream_t)stream, w,
                     f, flags_dev);
  OVN_HIP_CHECK(hipGetLastError());
  return OVN_OK;
}

extern "C" int ovn_tsdf_window_page_out(ovn_ctx* ctx, void* stream, const float* tsdf_dev, const float* weight_dev, int nx, int ny, int nz,
                                        const int32_t* base, int n, const int32_t* bricks_dev, const int32_t* slots_dev,
                                        float* pool_dev) {
  OVN_STORE_WINDOW("ovn_tsdf_window_page_out");
  OVN_REQUIRE(n >= 0, OVN_ERR_ARG, "ovn_tsdf_window_page_out: n %d < 0", n);
  if (n == 0) return OVN_OK;
  return page<true>("ovn_tsdf_window_page_out", ctx, stream, w, n, bricks_dev, slots_dev, pool_dev);
}

extern "C" int ovn_tsdf_window_page_in(ovn_ctx* ctx, void* stream, float* tsdf_dev, float* weight_dev, int nx, int ny, int nz,
                                       const int32_t* base, int n, const int32_t* bricks_dev, const int32_t* slots_dev,
                                       const float* pool_dev) {
  OVN_STORE_WINDOW("ovn_tsdf_window_page_in");
  OVN_REQUIRE(n >= 0, OVN_ERR_ARG, "ovn_tsdf_window_page_in: n %d < 0", n);
  if (n == 0) return OVN_OK;
  return page<false>("ovn_tsdf_window_page_in", ctx, stream, w, n, bricks_dev, slots_dev, pool_dev);
}
