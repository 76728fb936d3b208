// Weight gradients of the Delta head on frozen legs (generateNet.py:64-116 backwards), fp32, for gfx950, at any conv1size s and any
// feature width W of the context.  Notation: G = W // s, R = s G, H = G - 2; y = sigmoid(logit), t = target.
//
// Forward: fp32 operands and fp32 stage outputs, o1 (n, W, G, 64), o2 (n, G, G, 128) and o3 (n, H, H, 256) stay in scratch; the
// head precision mode plays no part.  Every sum of a stage is carried in fp64 and rounded once, so each stored value is the
// correctly rounded fp32 result of its fp32 inputs: the general path's c_conv1 kernel with a double accumulator
// (ovn_delta_generic_c1_wide, delta_head_generic.hip), then fwd_c2_kernel, fwd_c3_kernel and fwd_dense_kernel below.  Why not the
// fp32 sums of the inference kernels: the loss's slope makes dz sensitive to the logit (my_sigmoid_loss: d dz / d logit is of the
// order of dz itself times 24 / 4), and a logit summed in one fp32 chain over K = 128 s, 64 s, 1152 and 256 H^2 terms carries
// several times the rounding error of a blocked CPU sum; that error, not the backward pass, then dominates every gradient tensor.
//
// Backward of scale / n * sum_p loss(y_p, t_p), ReLU'(0) = 0, masks from the stored post-ReLU activations:
//   dz_p = scale / n * dloss/dy * y (1 - y)
//   Dense    gWd[k] = sum_p dz_p o3_p[k]            gbd = sum_p dz_p            dO3_p[k] = dz_p Wd[k] [o3_p[k] > 0]
//   c_conv3  gW3[kh,kw,ci,co] = sum_p sum_{y,x<H} o2_p[y+kh,x+kw,ci] dO3_p[y,x,co]      gb3[co] = sum dO3
//            dO2_p[u,v,ci] = [o2_p[u,v,ci] > 0] sum_{kh,kw,co} dO3_p[u-kh,v-kw,co] W3[kh,kw,ci,co]     (0 <= u-kh, v-kw < H)
//   c_conv2  gW2[di,o,ch] = sum_p sum_{ib,jb<G} o1_p[s ib+di,jb,o] dO2_p[ib,jb,ch]       gb2[ch] = sum dO2
//            dO1_p[s ib+di,jb,o] = sum_ch dO2_p[ib,jb,ch] W2[di,o,ch]                    rows i >= R: 0
//   c_conv1  gW1[dj,c,o] = sum_p sum_{i<R,jb<G} |l_p[i,c] - r_p[s jb+dj,c]| dO1_p[i,jb,o]  gb1[o] = sum dO1
//
// Kernels.  gW1 is the only large contraction ((128 s) x (R G) x 64 per pair, the FLOPs of the forward c_conv1): gw1_mfma_kernel runs
// it on v_mfma_f32_16x16x4_f32 with |l - r| formed in registers as the A operand, never stored.  Workgroup = (tap dj, pair block),
// wave = 16 channels x 64 outputs (four 16 x 16 accumulators), K walked as (pair, 4 rows i, jb).  128 s is a multiple of 16: no M
// edge; K rows are guarded by i < R with selects (EXEC stays full around the MFMAs).  gW2 / gW3 share one FMA kernel
// (atb_pairs_kernel: A^T B over the positions of a pair with a strided gather of A's rows), dO2 / dO1 read transposed copies of
// W3 / W2 made per call so that lanes run over the contiguous input channel.
//
// Determinism: no floating-point atomics.  Every kernel that sums over pairs writes ONE partial per block of OVN_GRAD_PAIR_BLOCK
// consecutive pairs (pairs in order inside it); grad_reduce_kernel adds the partials to the running sums in pair-block order.
// The call's chunks are whole pair blocks, so the bits depend neither on the chunking nor on the call.
//
// Bounds.  l rows read are i < R <= W; r rows read are s jb + dj <= s (G - 1) + s - 1 < R; o1 rows s ib + di < R; o2 rows
// (y + kh) G + x + kw <= G^2 - 1; dO3 positions are checked against [0, H); every store is guarded by its tensor's extent (pair
// p < pairs of the chunk, element < its count).
#include "ovn_internal.h"

namespace {

constexpr int FC = OVN_FEAT_C;    // 128
constexpr int O1 = OVN_C1_OUT;    // 64
constexpr int O2 = OVN_C2_OUT;    // 128
constexpr int O3 = OVN_C3_OUT;    // 256
constexpr int PB = OVN_GRAD_PAIR_BLOCK;

// Scratch of ovn_delta_head_grad_run for chunks of up to cmax pairs: the stage outputs o1 | o2 | o3, their gradients, per-pair dz /
// overlap / logits, the transposed kernels, the pair blocks' partials and (a call without a grad output) the running sums
struct GradScratch {
  float *o1 = nullptr, *o2 = nullptr, *o3 = nullptr, *dO1 = nullptr, *dO2 = nullptr, *dO3 = nullptr, *dz = nullptr, *ybuf = nullptr,
        *zbuf = nullptr, *w3t = nullptr, *w2t = nullptr, *part = nullptr, *grad = nullptr;
  GradScratch() = default;
  GradScratch(OvnCarver& c, size_t cmax, size_t o1e, size_t o2e, size_t o3e, size_t w3_elems, size_t w2_elems, size_t part_elems,
              size_t grad_elems) {
    o1 = c.take<float>(cmax * o1e);
    o2 = c.take<float>(cmax * o2e);
    o3 = c.take<float>(cmax * o3e);
    dO1 = c.take<float>(cmax * o1e);
    dO2 = c.take<float>(cmax * o2e);
    dO3 = c.take<float>(cmax * o3e);
    dz = c.take<float>(cmax);
    ybuf = c.take<float>(cmax);
    zbuf = c.take<float>(cmax);     // logits
    w3t = c.take<float>(w3_elems);
    w2t = c.take<float>(w2_elems);
    part = c.take<float>(part_elems);
    grad = c.take<float>(grad_elems);
  }
};

// out[t][b][a] = in[t][a][b]
__global__ __launch_bounds__(256) void transpose_kernel(const float* __restrict__ in, float* __restrict__ out, int T, int A, int B) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long long)T * A * B) return;
  const int a = (int)(idx % A);
  const int b = (int)((idx / A) % B);
  const int t = (int)(idx / ((long long)A * B));
  out[idx] = in[((size_t)t * A + a) * B + b];
}

// o2[pos][ch] = relu(b2[ch] + sum_{di < s, o < 64} o1[p][s ib + di][jb][o] W2[di][o][ch]), pos = (p, ib, jb); thread = (pos, ch), two
// positions per workgroup; rows read: s ib + di <= s (G - 1) + s - 1 < R
__global__ __launch_bounds__(256) void fwd_c2_kernel(const float* __restrict__ o1, const float* __restrict__ w2, const float* __restrict__ b2,
                                                     int s, int G, int W, long long npos, float* __restrict__ o2) {
  const long long pos = (long long)blockIdx.x * 2 + (threadIdx.x >> 7);
  if (pos >= npos) return;
  const int ch = (int)(threadIdx.x & 127);
  const int jb = (int)(pos % G), ib = (int)((pos / G) % G);
  const long long p = pos / ((long long)G * G);
  double acc = 0.0;
  for (int di = 0; di < s; ++di) {
    const float* a = o1 + (((size_t)p * W + (size_t)s * ib + di) * G + jb) * O1;
    const float* w = w2 + (size_t)di * O1 * O2 + ch;
#pragma unroll 8
    for (int o = 0; o < O1; ++o) acc = fma((double)a[o], (double)w[(size_t)o * O2], acc);
  }
  const float v = (float)(acc + (double)b2[ch]);
  o2[(size_t)pos * O2 + ch] = v > 0.f ? v : 0.f;
}

// o3[pos][co] = relu(b3[co] + sum_{kh, kw < 3, ci < 128} o2[p][y + kh][x + kw][ci] W3[kh][kw][ci][co]), pos = (p, y, x), y, x < H;
// workgroup = position, thread = co; rows / columns read: y + kh, x + kw <= H + 1 = G - 1
__global__ __launch_bounds__(256) void fwd_c3_kernel(const float* __restrict__ o2, const float* __restrict__ w3, const float* __restrict__ b3,
                                                     int G, int H, long long npos, float* __restrict__ o3) {
  const long long pos = blockIdx.x;
  if (pos >= npos) return;
  const int co = (int)threadIdx.x;
  const int x = (int)(pos % H), y = (int)((pos / H) % H);
  const long long p = pos / ((long long)H * H);
  double acc = 0.0;
  for (int t = 0; t < 9; ++t) {
    const float* a = o2 + (((size_t)p * G + y + t / 3) * G + x + t % 3) * O2;
    const float* w = w3 + (size_t)t * O2 * O3 + co;
#pragma unroll 8
    for (int ci = 0; ci < O2; ++ci) acc = fma((double)a[ci], (double)w[(size_t)ci * O3], acc);
  }
  const float v = (float)(acc + (double)b3[co]);
  o3[(size_t)pos * O3 + co] = v > 0.f ? v : 0.f;
}

// logit[p] = bd + <o3[p], wd> over K floats, overlap = sigmoid(logit): workgroup = pair, thread t sums k = t, t + 256, ... in fp64,
// the 256 sums join in a fixed tree
__global__ __launch_bounds__(256) void fwd_dense_kernel(const float* __restrict__ o3, const float* __restrict__ wd, const float* __restrict__ bd,
                                                        long long K, float* __restrict__ overlap, float* __restrict__ logit) {
  __shared__ double red[256];
  const float* x = o3 + (size_t)blockIdx.x * K;
  double acc = 0.0;
  for (long long k = threadIdx.x; k < K; k += 256) acc = fma((double)x[k], (double)wd[k], acc);
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float z = (float)(red[0] + (double)bd[0]);
    logit[blockIdx.x] = z;
    overlap[blockIdx.x] = (float)(1.0 / (1.0 + exp(-(double)z)));
  }
}

// thread = pair block: dz of its pairs, its partial of the Dense bias gradient and of the loss.  The scalar chain runs in fp64 from the
// forward's fp32 logit and is rounded once per result (one thread per pair block: it costs nothing)
__global__ __launch_bounds__(64) void loss_dz_kernel(const float* __restrict__ logit, const float* __restrict__ target, int np, int nb,
                                                     int loss, double coef, float* __restrict__ dz, float* __restrict__ partial,
                                                     long long stride, long long off_bd, long long off_loss) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= nb) return;
  float sl = 0.f, sd = 0.f;
  for (int q = 0; q < PB; ++q) {
    const int p = b * PB + q;
    if (p >= np) break;
    const double y = 1.0 / (1.0 + exp(-(double)logit[p])), d = y - (double)target[p];
    double l, dl;
    if (loss == 0) {   // my_sigmoid_loss: sigmoid(24 |y - t| - 6)
      l = 1.0 / (1.0 + exp(-(24.0 * fabs(d) - 6.0)));
      dl = 24.0 * l * (1.0 - l) * (d > 0.0 ? 1.0 : (d < 0.0 ? -1.0 : 0.0));
    } else {
      l = d * d;
      dl = 2.0 * d;
    }
    const float z = (float)(coef * dl * (y * (1.0 - y)));
    dz[p] = z;
    sd += z;
    sl += (float)(coef * l);
  }
  partial[b * stride + off_bd] = sd;
  partial[b * stride + off_loss] = sl;
}

// thread = (pair block, k): gWd partial and dO3 of the block's pairs
__global__ __launch_bounds__(256) void dense_grad_kernel(const float* __restrict__ o3, const float* __restrict__ wd,
                                                         const float* __restrict__ dz, int np, long long K, float* __restrict__ dO3,
                                                         float* __restrict__ partial, long long stride) {
  const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
  if (k >= K) return;
  const int b = blockIdx.y;
  const float w = wd[k];
  float acc = 0.f;
  for (int q = 0; q < PB; ++q) {
    const int p = b * PB + q;
    if (p >= np) break;
    const float v = o3[(size_t)p * K + k], z = dz[p];
    acc = fmaf(z, v, acc);
    dO3[(size_t)p * K + k] = v > 0.f ? z * w : 0.f;
  }
  partial[b * stride + k] = acc;
}

// Sum over the rows of a (rows, C) tensor per pair, per pair block: workgroup = (64 channels, pair block), four row lanes per
// channel (rows r = lane mod 4, pairs in order), joined as (0 + 1) + (2 + 3)
__global__ __launch_bounds__(256) void bias_grad_kernel(const float* __restrict__ D, long long pair_stride, long long rows, int C, int np,
                                                        float* __restrict__ partial, long long stride) {
  __shared__ float red[4][64];
  const int c = blockIdx.x * 64 + (threadIdx.x & 63), rl = threadIdx.x >> 6, b = blockIdx.y;
  float acc = 0.f;
  for (int q = 0; q < PB; ++q) {
    const int p = b * PB + q;
    if (p >= np) break;
    const float* d = D + (size_t)p * pair_stride + c;
    for (long long r = rl; r < rows; r += 4) acc += d[r * C];
  }
  red[rl][threadIdx.x & 63] = acc;
  __syncthreads();
  if (rl == 0) partial[b * stride + c] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

// out[t][a][c] = sum_{pairs of the block} sum_{y < PH, x < PW} A_p[(ya y + t / tw) AW + x + t % tw][a] B_p[y PW + x][c]
//   gW3: A = o2 (G, G, 128), B = dO3 (H, H, 256), ya = 1, tw = 3, T = 9;  gW2: A = o1 (W, G, 64), B = dO2 (G, G, 128), ya = s, tw = 1, T = s
// thread = (t, 8 channels a, c); a wave shares (t, a): its A loads are one address, its B loads one row segment
__global__ __launch_bounds__(256) void atb_pairs_kernel(const float* __restrict__ A, long long a_pair, int CA, int AW, int ya, int tw, int T,
                                                        const float* __restrict__ B, long long b_pair, int CB, int PH, int PW, int np,
                                                        float* __restrict__ partial, long long stride) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  const int c = (int)(idx % CB);
  const int a8 = (int)((idx / CB) % (CA / 8));
  const int t = (int)(idx / ((long long)CB * (CA / 8)));
  if (t >= T) return;
  const int b = blockIdx.y, oy = t / tw, ox = t % tw;
  float acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.f;
  for (int q = 0; q < PB; ++q) {
    const int p = b * PB + q;
    if (p >= np) break;
    const float* Ap = A + (size_t)p * a_pair + 8 * a8;
    const float* Bp = B + (size_t)p * b_pair + c;
    for (int y = 0; y < PH; ++y) {
      const float* ar = Ap + ((size_t)(ya * y + oy) * AW + ox) * CA;
      const float* br = Bp + (size_t)y * PW * CB;
#pragma unroll 2
      for (int x = 0; x < PW; ++x) {
        const f32x4 a0 = *reinterpret_cast<const f32x4*>(ar + (size_t)x * CA);
        const f32x4 a1 = *reinterpret_cast<const f32x4*>(ar + (size_t)x * CA + 4);
        const float bv = br[(size_t)x * CB];
        acc[0] = fmaf(a0[0], bv, acc[0]);
        acc[1] = fmaf(a0[1], bv, acc[1]);
        acc[2] = fmaf(a0[2], bv, acc[2]);
        acc[3] = fmaf(a0[3], bv, acc[3]);
        acc[4] = fmaf(a1[0], bv, acc[4]);
        acc[5] = fmaf(a1[1], bv, acc[5]);
        acc[6] = fmaf(a1[2], bv, acc[6]);
        acc[7] = fmaf(a1[3], bv, acc[7]);
      }
    }
  }
  float* out = partial + b * stride + ((size_t)t * CA + 8 * a8) * CB + c;
#pragma unroll
  for (int j = 0; j < 8; ++j) out[(size_t)j * CB] = acc[j];
}

// dO2: two waves per position (pair, u, v), lane = input channel ci; w3t[tap][co][ci]
__global__ __launch_bounds__(256) void c3_data_grad_kernel(const float* __restrict__ dO3, const float* __restrict__ w3t,
                                                           const float* __restrict__ o2, int G, int H, long long npos,
                                                           float* __restrict__ dO2) {
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const long long pos = (long long)blockIdx.x * 2 + (wave >> 1);
  if (pos >= npos) return;
  const int ci = ((wave & 1) << 6) + (int)(threadIdx.x & 63);
  const int v = (int)(pos % G), u = (int)((pos / G) % G);
  const long long p = pos / ((long long)G * G);
  float acc = 0.f;
  for (int kh = 0; kh < 3; ++kh) {
    const int yy = u - kh;
    if (yy < 0 || yy >= H) continue;
    for (int kw = 0; kw < 3; ++kw) {
      const int xx = v - kw;
      if (xx < 0 || xx >= H) continue;
      const float* d = dO3 + ((size_t)(p * H + yy) * H + xx) * O3;
      const float* w = w3t + (size_t)(kh * 3 + kw) * O3 * O2 + ci;
#pragma unroll 8
      for (int co = 0; co < O3; ++co) acc = fmaf(d[co], w[(size_t)co * O2], acc);
    }
  }
  const size_t e = (size_t)pos * O2 + ci;
  dO2[e] = o2[e] > 0.f ? acc : 0.f;
}

// dO1: one wave per (pair, row i, jb), lane = c_conv1 output o; w2t[di][ch][o]; rows i >= R get zeros
__global__ __launch_bounds__(256) void c2_data_grad_kernel(const float* __restrict__ dO2, const float* __restrict__ w2t, int s, int G, int W,
                                                           long long nitems, float* __restrict__ dO1) {
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const long long item = (long long)blockIdx.x * 4 + wave;
  if (item >= nitems) return;
  const int o = (int)(threadIdx.x & 63);
  const int jb = (int)(item % G), i = (int)((item / G) % W);
  const long long p = item / ((long long)G * W);
  float acc = 0.f;
  if (i < s * G) {
    const int ib = i / s, di = i - ib * s;
    const float* d = dO2 + ((size_t)(p * G + ib) * G + jb) * O2;
    const float* w = w2t + (size_t)di * O2 * O1 + o;
#pragma unroll 8
    for (int ch = 0; ch < O2; ++ch) acc = fmaf(d[ch], w[(size_t)ch * O1], acc);
  }
  dO1[(size_t)item * O1 + o] = acc;
}

// gW1 partial of one (tap dj, pair block): 8 waves, wave w = channels 16 w .. 16 w + 15 x all 64 outputs.
// MFMA 16x16x4 operands: A[m = lane & 15][k = lane >> 4] = |l[i0 + k][c0 + m] - r[s jb + dj][c0 + m]|, B[k][n = lane & 15] =
// dO1[i0 + k][jb][16 nt + n]; D: lane holds column n = lane & 15, rows m = 4 (lane >> 4) + j
__global__ __launch_bounds__(512) void gw1_mfma_kernel(const float* __restrict__ feats_l, const int32_t* __restrict__ lidx,
                                                       const float* __restrict__ feats_r, const int32_t* __restrict__ ridx,
                                                       const float* __restrict__ dO1, int s, int G, int W, int np,
                                                       float* __restrict__ partial, long long stride) {
  const int dj = blockIdx.x, b = blockIdx.y;
  const int lane = (int)(threadIdx.x & 63), c0 = 16 * (int)(threadIdx.x >> 6);
  const int m = lane & 15, kq = lane >> 4;
  const int R = s * G;
  f32x4 acc[4];
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) acc[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int q = 0; q < PB; ++q) {
    const int p = b * PB + q;
    if (p >= np) break;
    const float* L = feats_l + (size_t)(lidx ? lidx[p] : p) * W * FC + c0 + m;
    const float* Rr = feats_r + (size_t)(ridx ? ridx[p] : 0) * W * FC + (size_t)dj * FC + c0 + m;
    const float* D = dO1 + (size_t)p * W * G * O1 + m;
    for (int i0 = 0; i0 < R; i0 += 4) {
      const int i = i0 + kq;
      const bool ok = i < R;
      const int ic = ok ? i : 0;            // a row inside the tensor for the lanes past the K edge; their products are zeroed
      const float lv = L[(size_t)ic * FC];
      const float* dr = D + (size_t)ic * G * O1;
      for (int jb = 0; jb < G; ++jb) {
        const float rv = Rr[(size_t)s * jb * FC];
        const float a = ok ? fabsf(lv - rv) : 0.f;
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
          const float bv = ok ? dr[(size_t)jb * O1 + 16 * nt] : 0.f;
          acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bv, acc[nt], 0, 0, 0);
        }
      }
    }
  }
  float* out = partial + b * stride + ((size_t)dj * FC + c0 + 4 * kq) * O1 + m;
#pragma unroll
  for (int nt = 0; nt < 4; ++nt)
#pragma unroll
    for (int j = 0; j < 4; ++j) out[(size_t)j * O1 + 16 * nt] = acc[nt][j];
}

// running sums += the chunk's partials, in pair-block order; element `total` is the loss
__global__ __launch_bounds__(256) void grad_reduce_kernel(const float* __restrict__ partial, int nb, long long stride, long long total,
                                                          int first, float* __restrict__ grad, float* __restrict__ loss) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e > total) return;
  float* dst = e < total ? grad + e : loss;
  float acc = first ? 0.f : *dst;
  for (int b = 0; b < nb; ++b) acc += partial[b * stride + e];
  *dst = acc;
}

}  // namespace

void ovn_head_param_sizes_of(int s, int FW, int64_t* sizes8) {
  const int64_t G = FW / s, H = G - 2;
  sizes8[0] = (int64_t)FC * s * O1;
  sizes8[1] = O1;
  sizes8[2] = (int64_t)s * O1 * O2;
  sizes8[3] = O2;
  sizes8[4] = 9ll * O2 * O3;
  sizes8[5] = O3;
  sizes8[6] = H * H * O3;
  sizes8[7] = 1;
}

int ovn_delta_head_grad_run(ovn_ctx* ctx, int FW, const float* feats_l, const int32_t* lidx, const float* feats_r, const int32_t* ridx,
                            int64_t n, const float* target, int loss, float scale, float* grad, float* loss_out, float* overlap,
                            float* o2_out, float* o3_out, hipStream_t stream, float* dfeat_l, float* dfeat_r, bool forward_only) {
  const int s = ctx->head_s, G = ctx->head_g, H = G - 2;
  int64_t sz[8], off[8], total = 0;
  ovn_head_param_sizes_of(s, FW, sz);
  for (int t = 0; t < 8; ++t) {
    off[t] = total;
    total += sz[t];
  }
  const long long stride = (total + 1 + 63) & ~63ll;   // floats per pair block: the eight tensors, then the loss
  const size_t o1e = (size_t)FW * G * O1, o2e = (size_t)G * G * O2, o3e = (size_t)H * H * O3;
  const size_t fwd_pair = ovn_delta_generic_pair_bytes(FW, G);
  const size_t per_pair = fwd_pair + (o1e + o2e + o3e + 2) * sizeof(float) + (size_t)stride * sizeof(float) / PB + 64;
  int64_t chunk = (int64_t)((2ull << 30) / per_pair);
  if (ctx->head_chunk < chunk) chunk = ctx->head_chunk;
  chunk = chunk < PB ? PB : chunk / PB * PB;           // whole pair blocks: the partials do not depend on the chunking
  const int64_t cmax = n < chunk ? n : chunk;
  const int64_t nbmax = (cmax + PB - 1) / PB;
  GradScratch sc;   // (ovn_heads_feature_grad without head_grad_dev: the sums stay in scratch)
  int rc = ovn_ws_layout(ctx, stream, &sc, (size_t)cmax, o1e, o2e, o3e, (size_t)sz[4], (size_t)sz[2], (size_t)nbmax * stride,
                         (grad || forward_only) ? (size_t)0 : (size_t)total);
  if (rc) return rc;
  scratch_overwritten(ctx);
  float *o1 = sc.o1, *o2 = sc.o2, *o3 = sc.o3, *dO1 = sc.dO1, *dO2 = sc.dO2, *dO3 = sc.dO3, *dz = sc.dz, *ybuf = sc.ybuf, *zbuf = sc.zbuf,
        *w3t = sc.w3t, *w2t = sc.w2t, *part = sc.part;
  if (!grad && !forward_only) grad = sc.grad;
  // W3 (tap, ci, co) -> (tap, co, ci); W2 (di, o, ch) -> (di, ch, o)
  hipLaunchKernelGGL(transpose_kernel, dim3((unsigned)((sz[4] + 255) / 256)), dim3(256), 0, stream, ctx->head.w3raw, w3t, 9, O2, O3);
  hipLaunchKernelGGL(transpose_kernel, dim3((unsigned)((sz[2] + 255) / 256)), dim3(256), 0, stream, ctx->head.w2raw, w2t, s, O1, O2);
  OVN_HIP_CHECK(hipGetLastError());
  const double coef = (double)scale / (double)n;
  const size_t feat_elems = (size_t)FW * FC;
  for (int64_t p0 = 0; p0 < n; p0 += chunk) {
    const int np = (int)((n - p0 < chunk) ? (n - p0) : chunk);
    const int nb = (np + PB - 1) / PB;
    const float* fl = lidx ? feats_l : feats_l + (size_t)p0 * feat_elems;
    const int32_t* li = lidx ? lidx + p0 : nullptr;
    const int32_t* ri = ridx ? ridx + p0 : nullptr;
    float* y = overlap ? overlap + p0 : ybuf;
    {
      OvnProfScope ps(ctx, OVN_K_DELTA, stream);
      rc = ovn_delta_generic_c1_wide(ctx, FW, fl, li, feats_r, ri, np, o1, stream);
      if (rc) return rc;
      const long long npos2 = (long long)np * G * G, npos3 = (long long)np * H * H;
      hipLaunchKernelGGL(fwd_c2_kernel, dim3((unsigned)((npos2 + 1) / 2)), dim3(256), 0, stream, o1, ctx->head.w2raw, ctx->head.c2.bias, s, G, FW, npos2, o2);
      hipLaunchKernelGGL(fwd_c3_kernel, dim3((unsigned)npos3), dim3(256), 0, stream, o2, ctx->head.w3raw, ctx->head.c3.bias, G, H, npos3, o3);
      hipLaunchKernelGGL(fwd_dense_kernel, dim3((unsigned)np), dim3(256), 0, stream, o3, ctx->head.wd, ctx->head.bd, (long long)sz[6], y, zbuf);
    }
    if (o2_out) OVN_HIP_CHECK(hipMemcpyAsync(o2_out + (size_t)p0 * o2e, o2, (size_t)np * o2e * 4, hipMemcpyDeviceToDevice, stream));
    if (o3_out) OVN_HIP_CHECK(hipMemcpyAsync(o3_out + (size_t)p0 * o3e, o3, (size_t)np * o3e * 4, hipMemcpyDeviceToDevice, stream));
    if (forward_only) {
      OVN_HIP_CHECK(hipGetLastError());
      continue;
    }
    {   // loss, dz, Dense gradients, dO3
      OvnProfScope ps(ctx, OVN_K_DENSE, stream);
      hipLaunchKernelGGL(loss_dz_kernel, dim3((unsigned)((nb + 63) / 64)), dim3(64), 0, stream, zbuf, target + p0, np, nb, loss, coef, dz, part,
                         stride, (long long)off[7], (long long)total);
      hipLaunchKernelGGL(dense_grad_kernel, dim3((unsigned)((sz[6] + 255) / 256), (unsigned)nb), dim3(256), 0, stream, o3, ctx->head.wd, dz, np,
                         (long long)sz[6], dO3, part + off[6], stride);
    }
    {   // c_conv3: bias, kernel, dO2
      OvnProfScope ps(ctx, OVN_K_C3, stream);
      hipLaunchKernelGGL(bias_grad_kernel, dim3(O3 / 64, (unsigned)nb), dim3(256), 0, stream, dO3, (long long)o3e, (long long)H * H, O3, np,
                         part + off[5], stride);
      hipLaunchKernelGGL(atb_pairs_kernel, dim3((unsigned)(9 * (O2 / 8) * O3 / 256), (unsigned)nb), dim3(256), 0, stream, o2, (long long)o2e,
                         O2, G, 1, 3, 9, dO3, (long long)o3e, O3, H, H, np, part + off[4], stride);
      const long long npos = (long long)np * G * G;
      hipLaunchKernelGGL(c3_data_grad_kernel, dim3((unsigned)((npos + 1) / 2)), dim3(256), 0, stream, dO3, w3t, o2, G, H, npos, dO2);
    }
    {   // c_conv2: bias, kernel, dO1
      OvnProfScope ps(ctx, OVN_K_DELTA_C2, stream);
      hipLaunchKernelGGL(bias_grad_kernel, dim3(O2 / 64, (unsigned)nb), dim3(256), 0, stream, dO2, (long long)o2e, (long long)G * G, O2, np,
                         part + off[3], stride);
      hipLaunchKernelGGL(atb_pairs_kernel, dim3((unsigned)((s * (O1 / 8) * O2 + 255) / 256), (unsigned)nb), dim3(256), 0, stream, o1,
                         (long long)o1e, O1, G, s, 1, s, dO2, (long long)o2e, O2, G, G, np, part + off[2], stride);
      const long long nitems = (long long)np * FW * G;
      hipLaunchKernelGGL(c2_data_grad_kernel, dim3((unsigned)((nitems + 3) / 4)), dim3(256), 0, stream, dO2, w2t, s, G, FW, nitems, dO1);
    }
    {   // c_conv1: bias (rows i < R are the first R G rows of a pair's dO1), kernel on the matrix cores
      OvnProfScope ps(ctx, OVN_K_DELTA_PREP, stream);
      hipLaunchKernelGGL(bias_grad_kernel, dim3(O1 / 64, (unsigned)nb), dim3(256), 0, stream, dO1, (long long)o1e, (long long)s * G * G, O1,
                         np, part + off[1], stride);
      hipLaunchKernelGGL(gw1_mfma_kernel, dim3((unsigned)s, (unsigned)nb), dim3(512), 0, stream, fl, li, feats_r, ri, dO1, s, G, FW, np,
                         part + off[0], stride);
    }
    if (dfeat_l) {   // ovn_heads_feature_grad: the overlap loss's gradient down to both feature volumes (heads_feature_grad.hip)
      rc = ovn_delta_data_grad(ctx, FW, fl, li, feats_r, ri, dO1, np, dfeat_l + (size_t)p0 * feat_elems, dfeat_r + (size_t)p0 * feat_elems,
                               stream);
      if (rc) return rc;
    }
    hipLaunchKernelGGL(grad_reduce_kernel, dim3((unsigned)((total + 1 + 255) / 256)), dim3(256), 0, stream, part, nb, stride,
                       (long long)total, p0 == 0 ? 1 : 0, grad, loss_out);
    OVN_HIP_CHECK(hipGetLastError());
  }
  return OVN_OK;
}
