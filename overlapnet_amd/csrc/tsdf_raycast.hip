// A view of a TSDF volume from a pose: one ray per range-image pixel marched through the volume on a fixed lattice of samples, the
// first crossing from positive to non-positive tsdf is the hit (ovn_tsdf_raycast, ovn_tsdf_bricks).
// Compile this file with -ffp-contract=off: the result is DEFINED as a function of float32 operations that each round on their own
// (tests/_raycast_ref.py restates it in NumPy bit for bit), so no multiply may fuse with an add.
//
//   ray of pixel (py, px):  d_s, d_w and o exactly as csrc/render_mesh.hip forms them (the four host tables, R and o rounded to f32)
//   grid coordinates:       inv = 1 / voxel;  g_o = (o - origin) inv;  g_d = d_w inv
//   sample k:               t_k = min_range + (float)k step (one multiply, one add);  g = g_o + t_k g_d;  base corner floor(g)
//   valid:                  base corner in 0 .. n - 2 on every axis, all eight corner weights >= min_weight, F not a NaN
//   F:                      lerp(a, b, f) = a + f (b - a): four along x, two along y, one along z
//   march:                  positive valid sample -> remembered; invalid -> forgotten; F <= 0 ends the ray: a hit at
//                           t_p + (t_k - t_p) (F_p / (F_p - F)) when a positive sample is remembered, else empty
//
// One ray per lane, one wave per 8 x 8 pixel tile: a wave's rays stay within a few degrees of each other, so at a given k they sit in
// the same or neighbouring cells and their corner reads share cache lines.  A sample reads the brick byte first (when a mask is given),
// then the eight weights, then the eight tsdf values: in space nobody has seen it costs the byte, or the weights, alone.  Corners i and
// i + 1 are adjacent words (x is the fastest axis).  No LDS, no scratch, no atomics, no barriers: a pixel has one writer.
#include "ovn_internal.h"

namespace {

constexpr int TILE = 8;                 // a wave's pixel tile is TILE x TILE
constexpr int BRICK = 8;                // a mask byte covers BRICK^3 samples

struct RaycastArgs {
  const float* tsdf;           // (nz,ny,nx)
  const float* weight;
  const uint8_t* bricks;       // (bz,by,bx) or NULL
  const double* poses;         // (n,4,4) row-major, sensor to world
  const float *cos_az, *sin_az, *cos_pitch, *sin_pitch;
  float* range;
  float* vertex;
  long long pose0;             // first pose of this launch
  int nx, ny, nz, bx, by, H, W, tiles_x, tiles_per_scan, K;
  float ox, oy, oz, inv, min_weight, min_range, step;
  OvnRing ring;                // RING only
};

__device__ __forceinline__ float lerp1(float a, float b, float f) { return a + f * (b - a); }

// RING = false is the dense volume.  RING = true is the rolling window of ovn_tsdf_window_raycast (OvnRing, ovn_internal.h; DESIGN.md
// section 36): the base corner is valid in base .. base + n - 2, each of the eight corners is wrapped into its slot on its own, the
// brick byte is the one of the base corner's slot; the float32 operations are the dense ones
template <bool RING>
__global__ __launch_bounds__(64) void tsdf_raycast_kernel(RaycastArgs a) {
  const long long tile = blockIdx.x;
  const long long scan_local = tile / a.tiles_per_scan;
  const int tin = (int)(tile - scan_local * a.tiles_per_scan);
  const int ty = tin / a.tiles_x, tx = tin - ty * a.tiles_x;
  const int lane = threadIdx.x;
  const int y = ty * TILE + (lane >> 3), x = tx * TILE + (lane & 7);
  if (y >= a.H || x >= a.W) return;
  const long long scan = a.pose0 + scan_local;
  const long long q = (scan * a.H + y) * (long long)a.W + x;
  const double* P = a.poses + scan * 16;
  float R[9];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) R[i * 3 + j] = (float)P[i * 4 + j];
  const float ox = (float)P[3], oy = (float)P[7], oz = (float)P[11];
  float chk = (ox - ox) + (oy - oy) + (oz - oz);   // 0 when finite, NaN otherwise
#pragma unroll
  for (int i = 0; i < 9; ++i) chk += R[i] - R[i];
  const bool finite = (chk == 0.0f);
  const float cp = a.cos_pitch[y], sp = a.sin_pitch[y], ca = a.cos_az[x], sa = a.sin_az[x];
  const float dsx = cp * ca, dsy = cp * sa, dsz = sp;
  const float dwx = (R[0] * dsx + R[1] * dsy) + R[2] * dsz;
  const float dwy = (R[3] * dsx + R[4] * dsy) + R[5] * dsz;
  const float dwz = (R[6] * dsx + R[7] * dsy) + R[8] * dsz;
  const float gox = (ox - a.ox) * a.inv, goy = (oy - a.oy) * a.inv, goz = (oz - a.oz) * a.inv;
  const float gdx = dwx * a.inv, gdy = dwy * a.inv, gdz = dwz * a.inv;
  // n - 2 as a float may round once n exceeds 2^24 (n < 2^30: the other two axes hold 2 samples at least); the float test keeps the
  // conversion to int defined, the int test below decides
  // the window's bounds are exact as floats: |index| <= 2^20
  const int bi = RING ? a.ring.base[0] : 0, bj = RING ? a.ring.base[1] : 0, bk = RING ? a.ring.base[2] : 0;
  const int ti = bi + (a.nx - 2), tj = bj + (a.ny - 2), tk = bk + (a.nz - 2);
  const float botx = (float)bi, boty = (float)bj, botz = (float)bk;
  const float topx = (float)ti, topy = (float)tj, topz = (float)tk;
  const long long sy = a.nx, sz = (long long)a.nx * a.ny;
  bool have = false;           // the previous sample was valid and positive
  bool hit = false;
  float Fp = 0.0f, tp = 0.0f, hit_t = -1.0f;
  if (finite) {
    for (int k = 0; k < a.K; ++k) {
      const float t = a.min_range + (float)k * a.step;
      const float gx = gox + t * gdx, gy = goy + t * gdy, gz = goz + t * gdz;
      const float fx0 = floorf(gx), fy0 = floorf(gy), fz0 = floorf(gz);
      bool valid = (fx0 >= botx) && (fx0 <= topx) && (fy0 >= boty) && (fy0 <= topy) && (fz0 >= botz) && (fz0 <= topz);   // a NaN fails
      float F = 0.0f;
      if (valid) {
        int i = (int)fx0, j = (int)fy0, kk = (int)fz0;
        valid = (i <= ti) && (j <= tj) && (kk <= tk);
        // the corners' strides from the base corner: the next slot, or back to slot 0 from the last one
        long long dx = 1, dy = sy, dz = sz;
        if (RING && valid) {
          i = ovn_ring_slot(i, bi, a.ring.slot0[0], a.nx);
          j = ovn_ring_slot(j, bj, a.ring.slot0[1], a.ny);
          kk = ovn_ring_slot(kk, bk, a.ring.slot0[2], a.nz);
          if (i == a.nx - 1) dx = -(long long)(a.nx - 1);
          if (j == a.ny - 1) dy = -(long long)(a.ny - 1) * sy;
          if (kk == a.nz - 1) dz = -(long long)(a.nz - 1) * sz;
        }
        if (valid && a.bricks) valid = a.bricks[((long long)(kk >> 3) * a.by + (j >> 3)) * a.bx + (i >> 3)] != 0;
        if (valid) {
          const long long base = (long long)kk * sz + (long long)j * sy + i;
          const float* w = a.weight + base;
          const float w0 = w[0], w1 = w[dx], w2 = w[dy], w3 = w[dy + dx], w4 = w[dz], w5 = w[dz + dx], w6 = w[dz + dy], w7 = w[dz + dy + dx];
          const float mw = a.min_weight;
          valid = (w0 >= mw) && (w1 >= mw) && (w2 >= mw) && (w3 >= mw) && (w4 >= mw) && (w5 >= mw) && (w6 >= mw) && (w7 >= mw);
          if (valid) {
            const float* d = a.tsdf + base;
            const float fx = gx - fx0, fy = gy - fy0, fz = gz - fz0;
            const float c00 = lerp1(d[0], d[dx], fx);
            const float c10 = lerp1(d[dy], d[dy + dx], fx);
            const float c01 = lerp1(d[dz], d[dz + dx], fx);
            const float c11 = lerp1(d[dz + dy], d[dz + dy + dx], fx);
            const float c0 = lerp1(c00, c10, fy), c1 = lerp1(c01, c11, fy);
            F = lerp1(c0, c1, fz);
            valid = (F == F);            // neither > 0 nor <= 0: a NaN
          }
        }
      }
      if (!valid) {
        have = false;
      } else if (F > 0.0f) {
        have = true;
        Fp = F;
        tp = t;
      } else {
        if (have) {
          hit = true;
          hit_t = tp + (t - tp) * (Fp / (Fp - F));
        }
        break;
      }
    }
  }
  const float tt = hit ? hit_t : -1.0f;
  if (a.range) a.range[q] = tt;
  if (a.vertex) {
    const f32x4 v = hit ? (f32x4){tt * dsx, tt * dsy, tt * dsz, 1.0f} : (f32x4){-1.f, -1.f, -1.f, -1.f};
    *reinterpret_cast<f32x4*>(a.vertex + q * 4) = v;
  }
}

// one wave per run of 8 bricks along x: lane l owns x = 64 run + l through the 64 (dy, dz) rows of the bricks, so every load of the wave
// is 256 consecutive bytes; bits 8 g .. 8 g + 7 of the ballot belong to brick g of the run, and lane g < 8 writes that brick's byte
__global__ __launch_bounds__(64) void tsdf_bricks_kernel(const float* __restrict__ weight, int nx, int ny, int nz, int bx, int by,
                                                         int x_runs, float min_weight, uint8_t* __restrict__ bricks) {
  const long long b = blockIdx.x;
  const long long brow = b / x_runs;
  const int run = (int)(b - brow * x_runs);
  const int bk = (int)(brow / by), bj = (int)(brow - (long long)bk * by);
  const int lane = threadIdx.x;
  const int i = run * 64 + lane;
  bool any = false;
  if (i < nx) {
    for (int dz = 0; dz < BRICK; ++dz) {
      const int k = bk * BRICK + dz;
      if (k >= nz) break;                          // wave-uniform
      for (int dy = 0; dy < BRICK; ++dy) {
        const int j = bj * BRICK + dy;
        if (j >= ny) break;                        // wave-uniform
        any = any || (weight[((long long)k * ny + j) * nx + i] >= min_weight);
      }
    }
  }
  const unsigned long long m = __ballot(any);
  const int bi = run * 8 + lane;
  if (lane < 8 && bi < bx) bricks[((long long)bk * by + bj) * bx + bi] = ((m >> (8 * lane)) & 0xffull) != 0ull ? 1 : 0;
}

}  // namespace

// the number of samples k = 0, 1, .. with t_k = min_range + (float)k step < max_range in float32, counted up to `cap` + 1: t_k does
// not decrease with k (a rounded product and a rounded sum are monotone), so the count is the first k that fails, found by bisection
long long ovn_tsdf_raycast_samples(double min_range, double max_range, double step, long long cap) {
  const float mn = (float)min_range, mx = (float)max_range, st = (float)step;
  auto inside = [&](long long k) { return mn + (float)k * st < mx; };
  if (!inside(0)) return 0;
  if (inside(cap)) return cap + 1;
  long long lo = 0, hi = cap;          // inside(lo), !inside(hi)
  while (hi - lo > 1) {
    const long long mid = (lo + hi) / 2;
    if (inside(mid)) lo = mid; else hi = mid;
  }
  return hi;
}

int ovn_tsdf_raycast_forward(ovn_ctx* ctx, const float* tsdf, const float* weight, int nx, int ny, int nz, const double* origin,
                             double voxel, double min_weight, const uint8_t* bricks, const double* poses, int64_t n, int H, int W,
                             const float* cos_az, const float* sin_az, const float* cos_pitch, const float* sin_pitch, double min_range,
                             double step, int K, float* range, float* vertex, float* normal, float* stacked, int use_depth,
                             int use_normals, hipStream_t stream, const OvnRing* ring) {
  const bool want_post = normal || stacked;
  const bool need_vertex = normal || (stacked && use_normals);
  const long long HW = (long long)H * W;
  RaycastArgs a;
  a.tsdf = tsdf;
  a.weight = weight;
  a.bricks = bricks;
  a.poses = poses;
  a.cos_az = cos_az;
  a.sin_az = sin_az;
  a.cos_pitch = cos_pitch;
  a.sin_pitch = sin_pitch;
  a.nx = nx;
  a.ny = ny;
  a.nz = nz;
  a.bx = (nx + BRICK - 1) / BRICK;
  a.by = (ny + BRICK - 1) / BRICK;
  a.H = H;
  a.W = W;
  a.tiles_x = (W + TILE - 1) / TILE;
  a.tiles_per_scan = a.tiles_x * ((H + TILE - 1) / TILE);   // <= (H + 7)(W + 7) / 64 < 2^31
  a.K = K;
  a.ox = (float)origin[0];
  a.oy = (float)origin[1];
  a.oz = (float)origin[2];
  a.inv = 1.0f / (float)voxel;
  a.min_weight = (float)min_weight;
  a.min_range = (float)min_range;
  a.step = (float)step;
  a.ring = ring ? *ring : OvnRing{};
  const long long scans_per_launch = (1ll << 30) / a.tiles_per_scan > 0 ? (1ll << 30) / a.tiles_per_scan : 1;
  // the normal kernel reads range and vertex images: the caller's, or scratch of one launch's scans when it wants neither
  const long long slab_scans = n < scans_per_launch ? n : scans_per_launch;
  struct Scratch {
    float *range = nullptr, *vertex = nullptr;
    Scratch() = default;
    Scratch(OvnCarver& c, size_t nr, size_t nv) {
      range = nr ? c.take<float>(nr) : nullptr;
      vertex = nv ? c.take<float>(nv) : nullptr;
    }
  } sc;
  const bool tmp_range = want_post && !range, tmp_vertex = need_vertex && !vertex;
  if (tmp_range || tmp_vertex) {
    int rc = ovn_ws_layout(ctx, stream, &sc, tmp_range ? (size_t)(slab_scans * HW) : (size_t)0,
                           tmp_vertex ? (size_t)(slab_scans * HW * 4) : (size_t)0);
    if (rc) return rc;
    scratch_overwritten(ctx);
  }
  for (long long s0 = 0; s0 < n; s0 += scans_per_launch) {
    const long long ns = n - s0 < scans_per_launch ? n - s0 : scans_per_launch;
    // a scratch image holds this launch's scans only: shift its base so that the kernel's absolute index lands in it
    a.range = tmp_range ? sc.range - s0 * HW : range;
    a.vertex = tmp_vertex ? sc.vertex - s0 * HW * 4 : vertex;
    a.pose0 = s0;
    if (ring)
      hipLaunchKernelGGL(tsdf_raycast_kernel<true>, dim3((unsigned)(ns * a.tiles_per_scan)), dim3(64), 0, stream, a);
    else
      hipLaunchKernelGGL(tsdf_raycast_kernel<false>, dim3((unsigned)(ns * a.tiles_per_scan)), dim3(64), 0, stream, a);
    OVN_HIP_CHECK(hipGetLastError());
    if (want_post) {
      int rc = ovn_normals_stack_forward(a.range + s0 * HW, a.vertex ? a.vertex + s0 * HW * 4 : nullptr, (int)ns, H, W,
                                         normal ? normal + s0 * HW * 3 : nullptr,
                                         stacked ? stacked + s0 * HW * (use_depth + 3 * use_normals) : nullptr, use_depth,
                                         use_normals, stream);
      if (rc) return rc;
    }
  }
  return OVN_OK;
}

int ovn_tsdf_bricks_forward(const float* weight, int nx, int ny, int nz, double min_weight, uint8_t* bricks, hipStream_t stream) {
  const int bx = (nx + BRICK - 1) / BRICK, by = (ny + BRICK - 1) / BRICK, bz = (nz + BRICK - 1) / BRICK;
  const int x_runs = (bx + 7) / 8;
  const long long nb = (long long)x_runs * by * bz;   // <= the number of bricks <= the number of samples < 2^31
  hipLaunchKernelGGL(tsdf_bricks_kernel, dim3((unsigned)nb), dim3(64), 0, stream, weight, nx, ny, nz, bx, by, x_runs, (float)min_weight,
                     bricks);
  OVN_HIP_CHECK(hipGetLastError());
  return OVN_OK;
}
