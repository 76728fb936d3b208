// Virtual scans of a triangle mesh: one ray per range-image pixel, nearest hit (ovn_render_scans).
// Compile this file with -ffp-contract=off: the result is DEFINED as a function of float32 operations that each round on their own
// (a NumPy restatement reproduces it bit for bit, tests/_render_ref.py), so no multiply may fuse with an add.
//
//   ray of pixel (py, px):  d_s = (cp[py] ca[px], cp[py] sa[px], sp[py])  from the four host tables (no transcendental function here)
//                           d_w = (R[:,0] d_s.x + R[:,1] d_s.y) + R[:,2] d_s.z,  o = the pose's translation, both float32
//   ray_triangle():         Moeller-Trumbore, every dot product summed (a0 b0 + a1 b1) + a2 b2
//   winner of a pixel:      the smallest (t, triangle index) among the accepted hits
//
// Two routes share ray_triangle(), so they agree bit for bit on every (ray, triangle) pair both test:
//   render_exhaustive_kernel  every ray walks all T triangles in index order (the validation entry; loads are wave-uniform);
//   render_bvh_kernel         every ray walks an implicit complete binary tree of padded boxes over leaves of 4 triangles, near child
//                             first, pruned against its best t.  A culled node can hold no triangle that would change the winner
//                             (argument: DESIGN.md section 28), so the visiting order does not show in the result.
// One ray per lane, one wave per 8 x 8 pixel tile (a wave's rays stay within a few degrees of each other and share most of their
// path down the tree); partial tiles are guarded.  The traversal stack lives in LDS laid out [entry][lane] -- lane l of a wave reads
// and writes word e * 64 + l, bank l mod 64 whatever e is, so a wave's pushes and pops never conflict, and nothing is indexed
// dynamically in registers.  No atomics, no barriers: a pixel has one writer and a lane reads only its own stack words.
#include "ovn_internal.h"

namespace {

constexpr int TILE = 8;                 // a wave's pixel tile is TILE x TILE
constexpr int LEAF_TRIS = 4;            // triangles per leaf (OVN_RENDER_LEAF_TRIANGLES)
constexpr float SLAB_NEAR = 1.0f - 8.0f * 5.9604644775390625e-8f;   // 1 - 8 * 2^-24: entry distances are scaled DOWN by this,
constexpr float SLAB_FAR = 1.0f + 8.0f * 5.9604644775390625e-8f;    // exit distances UP (Ize's widened far bound, both ways)

struct RenderArgs {
  const float* vertices;       // (V,3)
  const int32_t* triangles;    // (T,3)
  const float* nodes;          // (2 NL, 8): lo.xyz, 0, hi.xyz, 0 of node i (root 1, children 2i and 2i + 1, leaves NL .. 2 NL - 1)
  const int32_t* order;        // (T): leaf j holds triangles order[4j .. 4j + 3]
  const double* poses;         // (n,4,4) row-major, sensor to world
  const float *cos_az, *sin_az, *cos_pitch, *sin_pitch;
  float* range;
  int32_t* tri_id;
  float* vertex;
  long long pose0;             // first pose of this launch
  int V, T, NL, H, W, tiles_x, tiles_per_scan;
  float max_range;
};

struct Ray {
  float ox, oy, oz, dx, dy, dz;
};

struct Hit {
  float t;
  int id;
};

// Moeller-Trumbore for triangle `tri` (0 <= tri < T); improves `best` when the hit is accepted and (t, tri) is smaller
__device__ __forceinline__ void ray_triangle(const RenderArgs& a, const Ray& r, int tri, Hit& best) {
  const int i0 = a.triangles[3ll * tri + 0], i1 = a.triangles[3ll * tri + 1], i2 = a.triangles[3ll * tri + 2];
  if ((unsigned)i0 >= (unsigned)a.V || (unsigned)i1 >= (unsigned)a.V || (unsigned)i2 >= (unsigned)a.V) return;   // never read
  const float* p0 = a.vertices + 3ll * i0;
  const float* p1 = a.vertices + 3ll * i1;
  const float* p2 = a.vertices + 3ll * i2;
  const float v0x = p0[0], v0y = p0[1], v0z = p0[2];
  const float e1x = p1[0] - v0x, e1y = p1[1] - v0y, e1z = p1[2] - v0z;
  const float e2x = p2[0] - v0x, e2y = p2[1] - v0y, e2z = p2[2] - v0z;
  const float px = r.dy * e2z - r.dz * e2y;                    // p = d x e2
  const float py = r.dz * e2x - r.dx * e2z;
  const float pz = r.dx * e2y - r.dy * e2x;
  const float det = (e1x * px + e1y * py) + e1z * pz;
  if (det == 0.0f || det != det) return;
  const float inv = 1.0f / det;
  const float sx = r.ox - v0x, sy = r.oy - v0y, sz = r.oz - v0z;
  const float u = ((sx * px + sy * py) + sz * pz) * inv;
  const float qx = sy * e1z - sz * e1y;                        // q = s x e1
  const float qy = sz * e1x - sx * e1z;
  const float qz = sx * e1y - sy * e1x;
  const float v = ((r.dx * qx + r.dy * qy) + r.dz * qz) * inv;
  const float t = ((e2x * qx + e2y * qy) + e2z * qz) * inv;
  const bool hit = (u >= 0.0f) && (v >= 0.0f) && (u + v <= 1.0f) && (t > 0.0f) && (t < a.max_range);
  if (hit && (t < best.t || (t == best.t && tri < best.id))) {
    best.t = t;
    best.id = tri;
  }
}

struct Pixel {
  long long q;     // index into the (n,H,W) images
  float dsx, dsy, dsz;
  bool finite;     // the pose's rotation and origin are finite in float32
};

// tile -> pixel and ray; false for a lane outside the image
__device__ __forceinline__ bool setup_ray(const RenderArgs& a, Pixel& px, Ray& r) {
  const long long tile = blockIdx.x;
  const long long scan_local = tile / a.tiles_per_scan;
  const int tin = (int)(tile - scan_local * a.tiles_per_scan);
  const int ty = tin / a.tiles_x, tx = tin - ty * a.tiles_x;
  const int lane = threadIdx.x;
  const int y = ty * TILE + (lane >> 3), x = tx * TILE + (lane & 7);
  if (y >= a.H || x >= a.W) return false;
  const long long scan = a.pose0 + scan_local;
  px.q = (scan * a.H + y) * (long long)a.W + x;
  const double* P = a.poses + scan * 16;
  float R[9];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) R[i * 3 + j] = (float)P[i * 4 + j];
  r.ox = (float)P[3];
  r.oy = (float)P[7];
  r.oz = (float)P[11];
  float chk = (r.ox - r.ox) + (r.oy - r.oy) + (r.oz - r.oz);   // 0 when finite, NaN otherwise
#pragma unroll
  for (int i = 0; i < 9; ++i) chk += R[i] - R[i];
  px.finite = (chk == 0.0f);
  const float cp = a.cos_pitch[y], sp = a.sin_pitch[y], ca = a.cos_az[x], sa = a.sin_az[x];
  px.dsx = cp * ca;
  px.dsy = cp * sa;
  px.dsz = sp;
  r.dx = (R[0] * px.dsx + R[1] * px.dsy) + R[2] * px.dsz;
  r.dy = (R[3] * px.dsx + R[4] * px.dsy) + R[5] * px.dsz;
  r.dz = (R[6] * px.dsx + R[7] * px.dsy) + R[8] * px.dsz;
  return true;
}

__device__ __forceinline__ void write_pixel(const RenderArgs& a, const Pixel& px, const Hit& best) {
  const bool hit = best.id >= 0;
  const float t = hit ? best.t : -1.0f;
  if (a.range) a.range[px.q] = t;
  if (a.tri_id) a.tri_id[px.q] = hit ? best.id : -1;
  if (a.vertex) {
    const f32x4 v = hit ? (f32x4){t * px.dsx, t * px.dsy, t * px.dsz, 1.0f} : (f32x4){-1.f, -1.f, -1.f, -1.f};
    *reinterpret_cast<f32x4*>(a.vertex + px.q * 4) = v;
  }
}

__global__ __launch_bounds__(64) void render_exhaustive_kernel(RenderArgs a) {
  Pixel px;
  Ray r;
  if (!setup_ray(a, px, r)) return;
  Hit best = {INFINITY, -1};
  if (px.finite)
    for (int tri = 0; tri < a.T; ++tri) ray_triangle(a, r, tri, best);
  write_pixel(a, px, best);
}

// Slab test of node `node` against the ray interval [0, limit]: the entry distance, or a negative number for a miss.  Each
// axis: (plane - o) * inv, three roundings with the one of inv; the entry side is scaled by SLAB_NEAR when positive and the exit side
// by SLAB_FAR, so the computed interval contains the exact one of the stored box.  A NaN (0 * inf: the origin on a slab plane of
// an axis the ray does not move along) fails both comparisons and leaves the interval as it is.  An empty leaf has lo > hi.
__device__ __forceinline__ float slab(const float* __restrict__ nodes, int node, const Ray& r, float ix, float iy, float iz, float limit) {
  const f32x4 lo = *reinterpret_cast<const f32x4*>(nodes + 8ll * node);
  const f32x4 hi = *reinterpret_cast<const f32x4*>(nodes + 8ll * node + 4);
  if (lo[0] > hi[0]) return -1.0f;
  float tn = 0.0f, tf = limit;
  {
    const float n = ((ix < 0.0f ? hi[0] : lo[0]) - r.ox) * ix, f = ((ix < 0.0f ? lo[0] : hi[0]) - r.ox) * ix;
    const float ns = n * SLAB_NEAR, fs = f * SLAB_FAR;
    tn = ns > tn ? ns : tn;
    tf = fs < tf ? fs : tf;
  }
  {
    const float n = ((iy < 0.0f ? hi[1] : lo[1]) - r.oy) * iy, f = ((iy < 0.0f ? lo[1] : hi[1]) - r.oy) * iy;
    const float ns = n * SLAB_NEAR, fs = f * SLAB_FAR;
    tn = ns > tn ? ns : tn;
    tf = fs < tf ? fs : tf;
  }
  {
    const float n = ((iz < 0.0f ? hi[2] : lo[2]) - r.oz) * iz, f = ((iz < 0.0f ? lo[2] : hi[2]) - r.oz) * iz;
    const float ns = n * SLAB_NEAR, fs = f * SLAB_FAR;
    tn = ns > tn ? ns : tn;
    tf = fs < tf ? fs : tf;
  }
  return tn > tf ? -1.0f : tn;
}

// dynamic LDS: stack_node[depth][64] then stack_t[depth][64]; depth = log2(NL) + 1 entries cover one deferred sibling per level
__global__ __launch_bounds__(64) void render_bvh_kernel(RenderArgs a, int depth) {
  extern __shared__ int lds[];
  Pixel px;
  Ray r;
  if (!setup_ray(a, px, r)) return;
  const int lane = threadIdx.x;
  int* stack_node = lds;
  float* stack_t = reinterpret_cast<float*>(lds + depth * 64);
  Hit best = {INFINITY, -1};
  if (px.finite) {
    const float ix = 1.0f / r.dx, iy = 1.0f / r.dy, iz = 1.0f / r.dz;
    int sp = 0;
    int node = 1;
    bool live = slab(a.nodes, 1, r, ix, iy, iz, a.max_range) >= 0.0f;
    while (live) {
      if (node < a.NL) {
        const float limit = best.t < a.max_range ? best.t : a.max_range;
        const int c0 = 2 * node;
        const float t0 = slab(a.nodes, c0, r, ix, iy, iz, limit);
        const float t1 = slab(a.nodes, c0 + 1, r, ix, iy, iz, limit);
        if (t0 >= 0.0f && t1 >= 0.0f) {
          const bool first0 = t0 <= t1;
          if (sp < depth) {       // always true for a tree of this depth; the guard keeps a wrong `depth` inside the LDS block
            stack_node[sp * 64 + lane] = first0 ? c0 + 1 : c0;
            stack_t[sp * 64 + lane] = first0 ? t1 : t0;
            ++sp;
          }
          node = first0 ? c0 : c0 + 1;
          continue;
        }
        if (t0 >= 0.0f || t1 >= 0.0f) {
          node = t0 >= 0.0f ? c0 : c0 + 1;
          continue;
        }
      } else {
        const long long first = (long long)(node - a.NL) * LEAF_TRIS;
#pragma unroll
        for (int k = 0; k < LEAF_TRIS; ++k) {
          if (first + k < a.T) {
            const int tri = a.order[first + k];
            if ((unsigned)tri < (unsigned)a.T) ray_triangle(a, r, tri, best);
          }
        }
      }
      // next deferred sibling that the best hit so far has not overtaken (an entry distance EQUAL to the best t stays: a triangle at
      // the same t with a smaller index must still be seen)
      live = false;
      while (sp > 0) {
        --sp;
        const float tn = stack_t[sp * 64 + lane];
        if (!(tn > best.t)) {
          node = stack_node[sp * 64 + lane];
          live = true;
          break;
        }
      }
    }
  }
  write_pixel(a, px, best);
}

}  // namespace

int ovn_render_scans_forward(ovn_ctx* ctx, const float* vertices, int V, const int32_t* triangles, int T, const float* nodes,
                             const int32_t* order, int NL, const double* poses, int64_t n, int H, int W, const float* cos_az,
                             const float* sin_az, const float* cos_pitch, const float* sin_pitch, double max_range, float* range,
                             int32_t* tri_id, float* vertex, float* normal, float* stacked, int use_depth, int use_normals,
                             hipStream_t stream) {
  const bool want_post = normal || stacked;
  const bool need_vertex = normal || (stacked && use_normals);
  const long long HW = (long long)H * W;
  RenderArgs a;
  a.vertices = vertices;
  a.triangles = triangles;
  a.nodes = nodes;
  a.order = order;
  a.poses = poses;
  a.cos_az = cos_az;
  a.sin_az = sin_az;
  a.cos_pitch = cos_pitch;
  a.sin_pitch = sin_pitch;
  a.tri_id = tri_id;
  a.V = V;
  a.T = T;
  a.NL = NL;
  a.H = H;
  a.W = W;
  a.tiles_x = (W + TILE - 1) / TILE;
  a.tiles_per_scan = a.tiles_x * ((H + TILE - 1) / TILE);   // <= (H + 7)(W + 7) / 64 < 2^31
  a.max_range = (float)max_range;
  int depth = 1;
  for (int m = NL; m > 1; m >>= 1) ++depth;
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
    // a scratch image holds this launch's scans only: shift its base so that the kernels' absolute index lands in it
    a.range = tmp_range ? sc.range - s0 * HW : range;
    a.vertex = tmp_vertex ? sc.vertex - s0 * HW * 4 : vertex;
    a.pose0 = s0;
    const dim3 grid((unsigned)(ns * a.tiles_per_scan));
    if (nodes) {
      hipLaunchKernelGGL(render_bvh_kernel, grid, dim3(64), (size_t)depth * 64 * 8, stream, a, depth);
    } else {
      hipLaunchKernelGGL(render_exhaustive_kernel, grid, dim3(64), 0, stream, a);
    }
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
