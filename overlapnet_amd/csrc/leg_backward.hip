// Backward pass of one leg layer (valid-padded NHWC convolution + bias + ReLU) on the fp32 matrix cores
// (v_mfma_f32_16x16x4_f32) for gfx950: the kernels behind ovn_leg_backward and ovn_debug_conv_grad.
//
// Per layer, with X (nb, H, W, Cin) its input, Y (nb, OH, OW, Cout) its stored post-ReLU output and dY = dL/dY * [Y > 0]:
//   bias     db[co]          = sum_{n, oy, ox} dY[n, oy, ox, co]
//   kernel   dW[ky,kx,ci,co] = sum_{n, oy, ox} X[n, oy sh + ky, ox sw + kx, ci] dY[n, oy, ox, co]
//   data     dX[n, y, x, ci] = sum_{ky, kx, co} dY[n, (y - ky) / sh, (x - kx) / sw, co] W[ky, kx, ci, co]     (exact divisions, in range)
//
// leg_mask_kernel    dY = [Y > 0] dL/dY for the top layer (every other layer's mask is applied by the data-gradient store below).
// leg_bgrad_kernel   column sums in fp64.  Workgroup = (64 channels, piece of pixels, scan block); four row groups, joined in order.
// leg_wgrad_kernel   GEMM  dW[k, co] = sum_p A[k, p] dY[p, co],  k = (ky, kx, ci) in Keras order, p = output pixel.  A is a transposed
//                    read of X: for one pixel the k of one ky are ONE contiguous run of kw Cin floats, so the workgroup stages 32 pixels
//                    x 64 k rows of X (each wave: 64 consecutive floats of one pixel) and 32 pixels x the column tile of dY in LDS and
//                    the MFMAs read both operands from there.  Workgroup = (64 k rows x up to 128 channels, piece of pixels, scan
//                    block); wave w owns k rows 16 w .. 16 w + 15.  Parallelism = output tiles x pieces x scan blocks.
// leg_dgrad_kernel   implicit GEMM, M = 16 input pixels of ONE input row per wave, N = Cin (tiles of up to 128), K = (ky, kx, co).  A row's
//                    valid ky are the same for the whole wave, so the others are skipped; a tap column that a pixel does not have
//                    ((x - kx) not a multiple of sw, or outside the output) has its A operand zeroed by a select: EXEC stays full
//                    around the MFMAs.  With channels last both operands are 16-byte loads: A = 4 consecutive co of dY, B = the same 4
//                    co of W[ky, kx, ci, :] in the Keras layout as registered.  Input rows / columns that no window covers come out
//                    as exact zeros (no tap is valid).  The store multiplies by [X > 0] when the layer below has a ReLU to pass.
// leg_dgrad_plain_kernel   the same sum in fp64, one thread per element: layers whose Cin is not a multiple of 16 (the first layer;
//                    only ovn_debug_conv_grad asks for its data gradient, nothing trains upstream of the leg).
//
// Accuracy: an fp32 MFMA accumulator runs over at most CHAIN = 256 terms (pixels of a weight gradient, (tap, co) of a data gradient),
// then it is added to an fp64 register; everything above that joins in fp64 and is rounded once.
// Determinism: no atomics.  A piece's fp64 partial goes to scratch; leg_join_kernel adds the partials onto the fp64 running sum in
// (scan block, piece) order, one thread per element.  Pieces are cut inside a scan block of OVN_LEG_GRAD_SCAN_BLOCK consecutive scans
// and their size depends on the layer's geometry alone, so the order of additions does not depend on how a call is sliced.
//
// Bounds.  wgrad: a pixel beyond the piece or the block gets base -1 and both operands 0 without a load; k rows >= K load nothing
// and store nothing; the X address of (pixel, k) is inside the pixel's window by construction.  dgrad: oy < OH by the row test, ox is
// 0 unless the tap is valid, co + 3 < Cout, ci < Cin (Cin a multiple of 16), stores guarded by x < W.  bgrad: pixels < those of the
// block, channel < Cout.
#include "ovn_internal.h"

namespace {

constexpr int SB = OVN_LEG_GRAD_SCAN_BLOCK;
constexpr int CHAIN = 256;    // terms of one fp32 accumulator chain
constexpr int PC = 32;        // pixels per LDS stage of the weight gradient
constexpr int TM = 64;        // k rows per workgroup of the weight gradient
constexpr int LDA = TM + 16;  // floats per staged pixel of A: the four pixel rows of an MFMA step fall 16 banks apart

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }

__global__ __launch_bounds__(256) void leg_mask_kernel(const float* __restrict__ dy, const float* __restrict__ y, float* __restrict__ out,
                                                       long long n) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) out[i] = y[i] > 0.f ? dy[i] : 0.f;
}

struct PieceArgs {
  int nb;              // scans of the slice
  int piece;           // pixels per workgroup
  long long out_px;    // OH * OW
};

__global__ __launch_bounds__(256) void leg_bgrad_kernel(const float* __restrict__ dy, double* __restrict__ part, int Cout, PieceArgs g) {
  __shared__ double red[4][64];
  const int co = 64 * (int)blockIdx.x + (int)(threadIdx.x & 63), rg = (int)(threadIdx.x >> 6);
  const int s0 = (int)blockIdx.z * SB;
  const long long Mb = (long long)(g.nb - s0 < SB ? g.nb - s0 : SB) * g.out_px;
  const long long p0 = (long long)blockIdx.y * g.piece;
  const long long p1 = p0 + g.piece < Mb ? p0 + g.piece : Mb;
  double s = 0.0;
  if (co < Cout)
    for (long long p = p0 + rg; p < p1; p += 4) s += (double)dy[((long long)s0 * g.out_px + p) * Cout + co];
  red[rg][threadIdx.x & 63] = s;
  __syncthreads();
  if (rg == 0 && co < Cout) {
    const int c = (int)threadIdx.x;
    part[((long long)blockIdx.z * gridDim.y + blockIdx.y) * Cout + co] = ((red[0][c] + red[1][c]) + red[2][c]) + red[3][c];
  }
}

struct WgArgs {
  const float* x;
  const float* dy;
  double* part;
  int W, Cin, OW, Cout, SH, SW, K, KWC, rowstride;
  long long in_scan;   // H * W * Cin
  PieceArgs g;
};

// MFMA 16x16x4: A[m = lane & 15][k = lane >> 4] = X[pixel 4 s + k][k row 16 wave + m], B[k][n = lane & 15] = dY[pixel 4 s + k][co];
// D: lane holds column n = lane & 15, rows 4 (lane >> 4) + j
template <int NT>
__global__ __launch_bounds__(256) void leg_wgrad_kernel(WgArgs a) {
  constexpr int LDB = NT == 1 ? 48 : 16 * NT + 16;   // as LDA: rows 16 banks apart (ds_read_b32 banks are modulo 32)
  constexpr int NA = NT >= 4 ? 1 : 2;     // accumulators per tile: a lone chain would wait out the MFMA's dependent latency
  __shared__ __attribute__((aligned(16))) float As[PC * LDA];
  __shared__ __attribute__((aligned(16))) float Bs[PC * LDB];
  __shared__ long long sbase[PC];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, m = lane & 15, kq = lane >> 4;
  const int ktiles = (a.K + TM - 1) / TM;
  const int k0 = ((int)blockIdx.x % ktiles) * TM, c0 = ((int)blockIdx.x / ktiles) * 16 * NT;
  const int s0 = (int)blockIdx.z * SB;
  const long long Mb = (long long)(a.g.nb - s0 < SB ? a.g.nb - s0 : SB) * a.g.out_px;
  const long long pb = (long long)blockIdx.y * a.g.piece;
  const long long pe = pb + a.g.piece < Mb ? pb + a.g.piece : Mb;
  const int krow = k0 + lane;             // staging: a wave reads 64 consecutive k rows of one pixel
  const bool kok = krow < a.K;
  long long koff = 0;
  if (kok) {
    const int ky = krow / a.KWC;
    koff = (long long)ky * a.rowstride + (krow - ky * a.KWC);
  }
  f32x4 acc[NT][NA];
  double dacc[NT][4];
#pragma unroll
  for (int j = 0; j < NT; ++j) {
#pragma unroll
    for (int t = 0; t < NA; ++t) acc[j][t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < 4; ++r) dacc[j][r] = 0.0;
  }
  auto flush = [&]() {
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      f32x4 v = acc[j][0];
      if (NA == 2) v = v + acc[j][NA - 1];
#pragma unroll
      for (int r = 0; r < 4; ++r) dacc[j][r] += (double)v[r];
#pragma unroll
      for (int t = 0; t < NA; ++t) acc[j][t] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
  };
  int staged = 0;
  for (long long p0 = pb; p0 < pe; p0 += PC) {
    if (tid < PC) {
      const long long p = p0 + tid;
      long long base = -1;
      if (p < pe) {
        const long long sc = p / a.g.out_px;
        const int r = (int)(p - sc * a.g.out_px);
        const int oy = r / a.OW, ox = r - oy * a.OW;
        base = (s0 + sc) * a.in_scan + ((long long)oy * a.SH * a.W + (long long)ox * a.SW) * a.Cin;
      }
      sbase[tid] = base;
    }
    __syncthreads();
    float av[PC / 4];
#pragma unroll
    for (int r = 0; r < PC / 4; ++r) {
      const long long b = sbase[wave + 4 * r];
      av[r] = (kok && b >= 0) ? a.x[b + koff] : 0.f;
    }
#pragma unroll
    for (int r = 0; r < PC / 4; ++r) As[(wave + 4 * r) * LDA + lane] = av[r];
    for (int slot = tid; slot < PC * 4 * NT; slot += 256) {
      const int pi = slot / (4 * NT), q = slot - pi * 4 * NT;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (p0 + pi < pe) v = ld4(a.dy + ((long long)s0 * a.g.out_px + p0 + pi) * a.Cout + c0 + 4 * q);
      *reinterpret_cast<f32x4*>(&Bs[pi * LDB + 4 * q]) = v;
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < PC / 4; ++s) {
      const float af = As[(4 * s + kq) * LDA + 16 * wave + m];
#pragma unroll
      for (int j = 0; j < NT; ++j)
        acc[j][s % NA] = __builtin_amdgcn_mfma_f32_16x16x4f32(af, Bs[(4 * s + kq) * LDB + 16 * j + m], acc[j][s % NA], 0, 0, 0);
    }
    staged += PC;
    if (staged == CHAIN) {
      flush();
      staged = 0;
    }
  }
  flush();
  double* out = a.part + ((long long)blockIdx.z * gridDim.y + blockIdx.y) * ((long long)a.K * a.Cout);
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int k = k0 + 16 * wave + 4 * kq + r;
      if (k < a.K) out[(long long)k * a.Cout + c0 + 16 * j + m] = dacc[j][r];
    }
}

struct DgArgs {
  const float* dy;
  const float* w;
  const float* mask;   // NULL, or the layer's input: the gradient passes where it is > 0
  float* dx;
  int H, W, Cin, OH, OW, Cout, SH, SW, KH, KW;
};

// MFMA 16x16x4: A[m = lane & 15][k = lane >> 4] = dY[pixel x0 + m, tap][co(k)], B[k][n = lane & 15] = W[tap][ci0 + n][co(k)], with the
// k of step e being co = co0 + 4 (lane >> 4) + e for both; D: lane holds channel n = lane & 15, pixels 4 (lane >> 4) + j
template <int NT>
__global__ __launch_bounds__(256) void leg_dgrad_kernel(DgArgs a) {
  constexpr int NA = NT >= 4 ? 1 : 2;
  const int lane = (int)(threadIdx.x & 63), wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int m = lane & 15, kq = lane >> 4;
  const int xtiles = (a.W + 63) / 64;
  const int x0 = ((int)blockIdx.x % xtiles) * 64 + 16 * wave, ci0 = ((int)blockIdx.x / xtiles) * 16 * NT;
  if (x0 >= a.W) return;                 // the whole wave; the kernel has no barrier
  const int y = (int)blockIdx.y;
  const long long n = blockIdx.z;
  const int x = x0 + m;
  f32x4 acc[NT][NA];
  double dacc[NT][4];
#pragma unroll
  for (int j = 0; j < NT; ++j) {
#pragma unroll
    for (int t = 0; t < NA; ++t) acc[j][t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < 4; ++r) dacc[j][r] = 0.0;
  }
  int terms = 0;
  for (int ky = 0; ky < a.KH; ++ky) {
    const int u = y - ky;
    if (u < 0 || u % a.SH != 0 || u / a.SH >= a.OH) continue;      // the same for every pixel of the row
    const int oy = u / a.SH;
    for (int kx = 0; kx < a.KW; ++kx) {
      const int t = x - kx;
      const bool ok = x < a.W && t >= 0 && t % a.SW == 0 && t / a.SW < a.OW;
      if (!__any(ok)) continue;
      const int ox = ok ? t / a.SW : 0;
      const float* ap = a.dy + ((n * a.OH + oy) * a.OW + ox) * a.Cout + 4 * kq;
      const float* bp = a.w + ((long long)(ky * a.KW + kx) * a.Cin + ci0 + m) * a.Cout + 4 * kq;
      for (int co0 = 0; co0 < a.Cout; co0 += 16) {
        const f32x4 ld = ld4(ap + co0);
        const f32x4 av = ok ? ld : f32x4{0.f, 0.f, 0.f, 0.f};
        f32x4 bv[NT];
#pragma unroll
        for (int j = 0; j < NT; ++j) bv[j] = ld4(bp + (long long)16 * j * a.Cout + co0);
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int j = 0; j < NT; ++j) acc[j][e % NA] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[e], bv[j][e], acc[j][e % NA], 0, 0, 0);
        terms += 16;
        if (terms == CHAIN) {
          terms = 0;
#pragma unroll
          for (int j = 0; j < NT; ++j) {
            f32x4 v = acc[j][0];
            if (NA == 2) v = v + acc[j][NA - 1];
#pragma unroll
            for (int r = 0; r < 4; ++r) dacc[j][r] += (double)v[r];
#pragma unroll
            for (int t2 = 0; t2 < NA; ++t2) acc[j][t2] = f32x4{0.f, 0.f, 0.f, 0.f};
          }
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    f32x4 v = acc[j][0];
    if (NA == 2) v = v + acc[j][NA - 1];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int xx = x0 + 4 * kq + r;
      if (xx < a.W) {
        const long long idx = ((n * a.H + y) * a.W + xx) * a.Cin + ci0 + 16 * j + m;
        float o = (float)(dacc[j][r] + (double)v[r]);
        if (a.mask) o = a.mask[idx] > 0.f ? o : 0.f;
        a.dx[idx] = o;
      }
    }
  }
}

__global__ __launch_bounds__(256) void leg_dgrad_plain_kernel(DgArgs a, long long total) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int ci = (int)(i % a.Cin);
    long long r = i / a.Cin;
    const int x = (int)(r % a.W);
    r /= a.W;
    const int y = (int)(r % a.H);
    const long long n = r / a.H;
    double s = 0.0;
    for (int ky = 0; ky < a.KH; ++ky) {
      const int u = y - ky;
      if (u < 0 || u % a.SH != 0 || u / a.SH >= a.OH) continue;
      for (int kx = 0; kx < a.KW; ++kx) {
        const int t = x - kx;
        if (t < 0 || t % a.SW != 0 || t / a.SW >= a.OW) continue;
        const float* dp = a.dy + ((n * a.OH + u / a.SH) * a.OW + t / a.SW) * a.Cout;
        const float* wp = a.w + ((long long)(ky * a.KW + kx) * a.Cin + ci) * a.Cout;
        for (int co = 0; co < a.Cout; ++co) s = fma((double)dp[co], (double)wp[co], s);
      }
    }
    float o = (float)s;
    if (a.mask) o = a.mask[i] > 0.f ? o : 0.f;
    a.dx[i] = o;
  }
}

// acc[e] += the partials of element e in (scan block, piece) order
__global__ __launch_bounds__(256) void leg_join_kernel(const double* __restrict__ part, int nparts, long long elems, double* __restrict__ acc) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= elems) return;
  double s = acc[e];
  for (int p = 0; p < nparts; ++p) s += part[(long long)p * elems + e];
  acc[e] = s;
}

__global__ __launch_bounds__(256) void leg_round_kernel(const double* __restrict__ acc, float* __restrict__ out, long long n) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e < n) out[e] = (float)acc[e];
}

// pixels per workgroup of the two reductions: whole fp32 chains, more of them where a scan block has more pixels (geometry alone)
int piece_of(long long out_px) {
  long long nsub = (SB * out_px) / (16 * CHAIN);
  nsub = nsub < 1 ? 1 : (nsub > 8 ? 8 : nsub);
  return (int)(CHAIN * nsub);
}

int tile_of(int c16) { return c16 % 8 == 0 ? 8 : (c16 % 4 == 0 ? 4 : (c16 % 2 == 0 ? 2 : 1)); }

unsigned blocks_for(long long n) {
  const long long b = (n + 255) / 256;
  return (unsigned)(b < 1 ? 1 : (b > 65535 ? 65535 : b));
}

}  // namespace

size_t ovn_leg_grad_part_bytes(const OvnConvLayer& L, int h, int w, int nb) {
  const long long out_px = (long long)((h - L.kh) / L.sh + 1) * ((w - L.kw) / L.sw + 1);
  const long long pieces = (SB * out_px + piece_of(out_px) - 1) / piece_of(out_px);
  const long long blocks = (nb + SB - 1) / SB;
  return (size_t)(blocks * pieces) * (size_t)L.kh * L.kw * L.cin * L.cout * sizeof(double);
}

int ovn_leg_mask_forward(const float* dy, const float* y, float* out, long long n, hipStream_t stream) {
  if (n <= 0) return OVN_OK;
  hipLaunchKernelGGL(leg_mask_kernel, dim3(blocks_for(n)), dim3(256), 0, stream, dy, y, out, n);
  OVN_HIP_CHECK(hipGetLastError());
  return OVN_OK;
}

int ovn_leg_grad_round(const double* acc, float* out, long long n, hipStream_t stream) {
  if (n <= 0) return OVN_OK;
  hipLaunchKernelGGL(leg_round_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, acc, out, n);
  OVN_HIP_CHECK(hipGetLastError());
  return OVN_OK;
}

int ovn_leg_layer_backward(const OvnConvLayer& L, const float* x, const float* dym, int nb, int h, int w, float* dx, const float* mask,
                           double* acc_kernel, double* acc_bias, double* part, hipStream_t stream) {
  OVN_REQUIRE(L.wraw != nullptr, OVN_ERR_STATE, "layer %s keeps no raw kernel", L.name.c_str());
  OVN_REQUIRE(h >= L.kh && w >= L.kw, OVN_ERR_ARG, "layer %s: input %dx%d smaller than kernel", L.name.c_str(), h, w);
  OVN_REQUIRE(L.cout % 16 == 0, OVN_ERR_ARG, "layer %s: cout=%d must be a multiple of 16", L.name.c_str(), L.cout);
  if (nb <= 0) return OVN_OK;
  const int OH = (h - L.kh) / L.sh + 1, OW = (w - L.kw) / L.sw + 1;
  const int K = L.kh * L.kw * L.cin;
  PieceArgs g;
  g.nb = nb;
  g.out_px = (long long)OH * OW;
  g.piece = piece_of(g.out_px);
  const unsigned pieces = (unsigned)((SB * g.out_px + g.piece - 1) / g.piece), blocks = (unsigned)((nb + SB - 1) / SB);
  OVN_REQUIRE(pieces <= 65535 && blocks <= 65535, OVN_ERR_ARG, "layer %s: %u pieces x %u scan blocks exceed the grid", L.name.c_str(),
              pieces, blocks);
  if (acc_bias) {
    hipLaunchKernelGGL(leg_bgrad_kernel, dim3((unsigned)((L.cout + 63) / 64), pieces, blocks), dim3(256), 0, stream, dym, part, L.cout, g);
    hipLaunchKernelGGL(leg_join_kernel, dim3((unsigned)((L.cout + 255) / 256)), dim3(256), 0, stream, part, (int)(pieces * blocks),
                       (long long)L.cout, acc_bias);
  }
  if (acc_kernel) {
    WgArgs a;
    a.x = x;
    a.dy = dym;
    a.part = part;
    a.W = w;
    a.Cin = L.cin;
    a.OW = OW;
    a.Cout = L.cout;
    a.SH = L.sh;
    a.SW = L.sw;
    a.K = K;
    a.KWC = L.kw * L.cin;
    a.rowstride = w * L.cin;
    a.in_scan = (long long)h * w * L.cin;
    a.g = g;
    const int nt = tile_of(L.cout / 16);
    const dim3 grid((unsigned)(((K + TM - 1) / TM) * (L.cout / (16 * nt))), pieces, blocks);
    switch (nt) {
      case 8: hipLaunchKernelGGL(leg_wgrad_kernel<8>, grid, dim3(256), 0, stream, a); break;
      case 4: hipLaunchKernelGGL(leg_wgrad_kernel<4>, grid, dim3(256), 0, stream, a); break;
      case 2: hipLaunchKernelGGL(leg_wgrad_kernel<2>, grid, dim3(256), 0, stream, a); break;
      default: hipLaunchKernelGGL(leg_wgrad_kernel<1>, grid, dim3(256), 0, stream, a); break;
    }
    const long long elems = (long long)K * L.cout;
    hipLaunchKernelGGL(leg_join_kernel, dim3((unsigned)((elems + 255) / 256)), dim3(256), 0, stream, part, (int)(pieces * blocks), elems,
                       acc_kernel);
  }
  if (dx) {
    DgArgs d;
    d.dy = dym;
    d.w = L.wraw;
    d.mask = mask;
    d.dx = dx;
    d.H = h;
    d.W = w;
    d.Cin = L.cin;
    d.OH = OH;
    d.OW = OW;
    d.Cout = L.cout;
    d.SH = L.sh;
    d.SW = L.sw;
    d.KH = L.kh;
    d.KW = L.kw;
    if (L.cin % 16 == 0) {
      OVN_REQUIRE(h <= 65535 && nb <= 65535, OVN_ERR_ARG, "layer %s: %d rows x %d scans exceed the grid", L.name.c_str(), h, nb);
      const int nt = tile_of(L.cin / 16);
      const dim3 grid((unsigned)(((w + 63) / 64) * (L.cin / (16 * nt))), (unsigned)h, (unsigned)nb);
      switch (nt) {
        case 8: hipLaunchKernelGGL(leg_dgrad_kernel<8>, grid, dim3(256), 0, stream, d); break;
        case 4: hipLaunchKernelGGL(leg_dgrad_kernel<4>, grid, dim3(256), 0, stream, d); break;
        case 2: hipLaunchKernelGGL(leg_dgrad_kernel<2>, grid, dim3(256), 0, stream, d); break;
        default: hipLaunchKernelGGL(leg_dgrad_kernel<1>, grid, dim3(256), 0, stream, d); break;
      }
    } else {
      const long long total = (long long)nb * h * w * L.cin;
      hipLaunchKernelGGL(leg_dgrad_plain_kernel, dim3(blocks_for(total)), dim3(256), 0, stream, d, total);
    }
  }
  OVN_HIP_CHECK(hipGetLastError());
  return OVN_OK;
}
