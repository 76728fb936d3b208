// SE(3) pose-graph optimization in fp64 (ovn_pose_graph_*; include/ovn_hip.h): linearization of the edges,
// block-sparse preconditioned conjugate gradients with a block-Jacobi or an odometry-chain preconditioner, and the retraction; and the
// chain-plus-loops inverse (ovn_pose_graph_loops_*; tests/_pose_graph_loops_ref.py): the exact inverse of the
// undamped Hessian of a chain plus L loop edges, with a dense Cholesky factorization of order 6 L; and the marginal covariances that
// inverse's diagonal blocks are (ovn_pose_graph_marginals; tests/_pose_graph_marginals_ref.py).
// No atomics, and no workgroup waits on another inside a launch.  A node sums over its incidence list in list order.
// Reductions: every dot product and maximum over nodes is a fixed tree -- 256 lanes halving inside a workgroup (pg_wg_sum, pg_wg_max),
// then ONE workgroup over the per-workgroup partials, lane t taking partials t, t + 256, ... in order (pg_partial_sum, pg_partial_max).
// Scans: every prefix sum over the chain is the one scan of "the scan" below, three launches: Hillis-Steele inside blocks of 256
// (pg_block_scan6), the block totals added in block order by one lane per component, and the offset added to every block but the first.
// Built without FMA contraction: tests/_pose_graph_ref.py states the same operations one by one.
#include "ovn_internal.h"

namespace {

constexpr int PG_B = 256;              // threads per workgroup, elements per scan block
constexpr double PG_SERIES_X = 1e-2;   // theta^2 below which the coefficient series are used

// record slots (OVN_POSE_GRAPH_RECORD doubles)
enum { R_COST = 0, R_BAD = 1, R_CHOL = 2, R_GMAX = 3, R_ITER = 4, R_REL = 5, R_CONV = 6, R_BREAK = 7, R_RZ = 8, R_RZ0 = 9, R_ALPHA = 10,
       R_BETA = 11, R_DMAX = 12, R_LPIV = 13, R_LOUT = 14, R_MOUT = 15 };

// the carve of the three workspace layouts below: the next n doubles (NULL when only measuring), rounded up to an even count
struct PgTake {
  double* base;
  size_t o = 0;
  double* operator()(size_t n) {
    double* q = base ? base + o : nullptr;
    o += (n + 1) & ~(size_t)1;
    return q;
  }
};

struct PgWs {   // the caller's workspace, in doubles
  double *eg, *part_e, *part_n, *part_c, *r, *z, *q, *p[2], *sa, *sb, *bsum;
  size_t total;
  PgWs(double* base, int64_t N, int64_t E) {
    const int64_t nbn = (N + PG_B - 1) / PG_B, nbe = (E + PG_B - 1) / PG_B;
    PgTake take{base};
    part_n = take(2 * nbn);   // the node-sized parts first: their places do not depend on E
    part_c = take(nbn);
    r = take(6 * N);
    z = take(6 * N);
    q = take(6 * N);
    p[0] = take(6 * N);
    p[1] = take(6 * N);
    sa = take(6 * N);
    sb = take(6 * N);
    bsum = take(12 * nbn);
    part_e = take(2 * nbe);
    eg = take(12 * E);
    total = take.o;
  }
};

// ---- small fixed-size algebra, every sum in index order ---------------------------------------------------------------------------------
__device__ __forceinline__ void m3_mul(const double* a, const double* b, double* c) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) c[i * 3 + j] = (a[i * 3] * b[j] + a[i * 3 + 1] * b[3 + j]) + a[i * 3 + 2] * b[6 + j];
}
__device__ __forceinline__ void m3_tmul(const double* a, const double* b, double* c) {   // a' b
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) c[i * 3 + j] = (a[i] * b[j] + a[3 + i] * b[3 + j]) + a[6 + i] * b[6 + j];
}
__device__ __forceinline__ void m3_vec(const double* a, const double* v, double* o) {
#pragma unroll
  for (int i = 0; i < 3; ++i) o[i] = (a[i * 3] * v[0] + a[i * 3 + 1] * v[1]) + a[i * 3 + 2] * v[2];
}
__device__ __forceinline__ void m3_tvec(const double* a, const double* v, double* o) {   // a' v
#pragma unroll
  for (int i = 0; i < 3; ++i) o[i] = (a[i] * v[0] + a[3 + i] * v[1]) + a[6 + i] * v[2];
}
__device__ __forceinline__ void m3_hat(const double* w, double* h) {
  h[0] = 0.0; h[1] = -w[2]; h[2] = w[1];
  h[3] = w[2]; h[4] = 0.0; h[5] = -w[0];
  h[6] = -w[1]; h[7] = w[0]; h[8] = 0.0;
}
__device__ __forceinline__ void m6_mul(const double* a, const double* b, double* c) {
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      double s = a[i * 6] * b[j];
#pragma unroll
      for (int k = 1; k < 6; ++k) s = s + a[i * 6 + k] * b[k * 6 + j];
      c[i * 6 + j] = s;
    }
}
__device__ __forceinline__ void m6_tmul(const double* a, const double* b, double* c) {   // a' b
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      double s = a[i] * b[j];
#pragma unroll
      for (int k = 1; k < 6; ++k) s = s + a[k * 6 + i] * b[k * 6 + j];
      c[i * 6 + j] = s;
    }
}
__device__ __forceinline__ void m6_mult(const double* a, const double* b, double* c) {   // a b'
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      double s = a[i * 6] * b[j * 6];
#pragma unroll
      for (int k = 1; k < 6; ++k) s = s + a[i * 6 + k] * b[j * 6 + k];
      c[i * 6 + j] = s;
    }
}
__device__ __forceinline__ void m6_vec(const double* a, const double* v, double* o) {
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    double s = a[i * 6] * v[0];
#pragma unroll
    for (int k = 1; k < 6; ++k) s = s + a[i * 6 + k] * v[k];
    o[i] = s;
  }
}
__device__ __forceinline__ void m6_tvec(const double* a, const double* v, double* o) {   // a' v
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    double s = a[i] * v[0];
#pragma unroll
    for (int k = 1; k < 6; ++k) s = s + a[k * 6 + i] * v[k];
    o[i] = s;
  }
}
__device__ __forceinline__ double v6_dot(const double* a, const double* b) {
  double s = a[0] * b[0];
#pragma unroll
  for (int k = 1; k < 6; ++k) s = s + a[k] * b[k];
  return s;
}
__device__ __forceinline__ void ld6(const double* p, double* v) {
#pragma unroll
  for (int k = 0; k < 6; ++k) v[k] = p[k];
}
__device__ __forceinline__ void st6(double* p, const double* v) {
#pragma unroll
  for (int k = 0; k < 6; ++k) p[k] = v[k];
}
__device__ __forceinline__ void ld36(const double* p, double* v) {
#pragma unroll
  for (int k = 0; k < 36; ++k) v[k] = p[k];
}
__device__ __forceinline__ void st36(double* p, const double* v) {
#pragma unroll
  for (int k = 0; k < 36; ++k) p[k] = v[k];
}

// a = sin t / t, b = (1 - cos t) / t^2, c1 = (t - sin t) / t^3, c2 = (t^2 + 2 cos t - 2) / (2 t^4),
// c3 = (2 t - 3 sin t + t cos t) / (2 t^5), e = 1 / t^2 - (1 + cos t) / (2 t sin t); x = t^2
struct PgCoef {
  double a, b, c1, c2, c3, e;
};
__device__ __forceinline__ PgCoef pg_coeffs(double x) {
  PgCoef c;
  if (x < PG_SERIES_X) {
    c.a = 1.0 + x * (-1.0 / 6 + x * (1.0 / 120 + x * (-1.0 / 5040 + x * (1.0 / 362880))));
    c.b = 0.5 + x * (-1.0 / 24 + x * (1.0 / 720 + x * (-1.0 / 40320 + x * (1.0 / 3628800))));
    c.c1 = 1.0 / 6 + x * (-1.0 / 120 + x * (1.0 / 5040 + x * (-1.0 / 362880 + x * (1.0 / 39916800))));
    c.c2 = 1.0 / 24 + x * (-1.0 / 720 + x * (1.0 / 40320 + x * (-1.0 / 3628800 + x * (1.0 / 479001600))));
    c.c3 = 1.0 / 120 + x * (-2.0 / 5040 + x * (3.0 / 362880 + x * (-4.0 / 39916800 + x * (5.0 / 6227020800.0))));
    c.e = 1.0 / 12 + x * (1.0 / 720 + x * (1.0 / 30240 + x * (1.0 / 1209600 + x * (1.0 / 47900160))));
    return c;
  }
  const double t = sqrt(x), s = sin(t), cs = cos(t);
  c.a = s / t;
  c.b = (1.0 - cs) / x;
  c.c1 = (t - s) / (x * t);
  c.c2 = ((x + 2.0 * cs) - 2.0) / ((2.0 * x) * x);
  c.c3 = ((2.0 * t - 3.0 * s) + t * cs) / (((2.0 * x) * x) * t);
  c.e = 1.0 / x - (1.0 + cs) / ((2.0 * t) * s);
  return c;
}

// a pose as rotation (row-major 3 x 3) and translation, from the top three rows of a (4,4) matrix
__device__ __forceinline__ void pg_load_pose(const double* T, double* R, double* t) {
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    R[i * 3] = T[i * 4]; R[i * 3 + 1] = T[i * 4 + 1]; R[i * 3 + 2] = T[i * 4 + 2];
    t[i] = T[i * 4 + 3];
  }
}
__device__ __forceinline__ bool pg_finite12(const double* R, const double* t) {
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < 9; ++k) s += R[k] * 0.0;
#pragma unroll
  for (int k = 0; k < 3; ++k) s += t[k] * 0.0;
  return s == 0.0;   // NaN and Inf give NaN
}
// A^-1 B: R = Ra' Rb, t = Ra' (tb - ta)
__device__ __forceinline__ void pg_rel(const double* Ra, const double* ta, const double* Rb, const double* tb, double* R, double* t) {
  m3_tmul(Ra, Rb, R);
  const double d[3] = {tb[0] - ta[0], tb[1] - ta[1], tb[2] - ta[2]};
  m3_tvec(Ra, d, t);
}
// Log of (R, t): (v, omega)
__device__ __forceinline__ void pg_log(const double* R, const double* t, double* xi) {
  const double ax[3] = {0.5 * (R[7] - R[5]), 0.5 * (R[2] - R[6]), 0.5 * (R[3] - R[1])};
  const double sn = sqrt((ax[0] * ax[0] + ax[1] * ax[1]) + ax[2] * ax[2]);
  const double cs = 0.5 * (((R[0] + R[4]) + R[8]) - 1.0);
  const double th = atan2(sn, cs);
  const double x = th * th;
  const double k = x < PG_SERIES_X ? 1.0 / pg_coeffs(x).a : th / sn;
  const double w[3] = {k * ax[0], k * ax[1], k * ax[2]};
  const double x2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2];
  const double e = pg_coeffs(x2).e;
  double W[9], WW[9], V[9];
  m3_hat(w, W);
  m3_mul(W, W, WW);
#pragma unroll
  for (int q = 0; q < 9; ++q) V[q] = (((q % 4 == 0) ? 1.0 : 0.0) - 0.5 * W[q]) + e * WW[q];
  m3_vec(V, t, xi);
  xi[3] = w[0]; xi[4] = w[1]; xi[5] = w[2];
}
// Exp of (v, omega): rotation and translation
__device__ __forceinline__ void pg_exp(const double* xi, double* R, double* t) {
  const double* w = xi + 3;
  const double x = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2];
  const PgCoef c = pg_coeffs(x);
  double W[9], WW[9], V[9];
  m3_hat(w, W);
  m3_mul(W, W, WW);
#pragma unroll
  for (int q = 0; q < 9; ++q) {
    const double id = (q % 4 == 0) ? 1.0 : 0.0;
    R[q] = (id + c.a * W[q]) + c.b * WW[q];
    V[q] = (id + c.b * W[q]) + c.c1 * WW[q];
  }
  m3_vec(V, xi, t);
}
// Ad(R, t) = [[R, t^ R], [0, R]]
__device__ __forceinline__ void pg_adjoint(const double* R, const double* t, double* Ad) {
  double H[9], HR[9];
  m3_hat(t, H);
  m3_mul(H, R, HR);
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      Ad[i * 6 + j] = R[i * 3 + j];
      Ad[i * 6 + 3 + j] = HR[i * 3 + j];
      Ad[(i + 3) * 6 + j] = 0.0;
      Ad[(i + 3) * 6 + 3 + j] = R[i * 3 + j];
    }
}
// Ad(T^-1) of T = (R, t): T^-1 = (R', -(R' t))
__device__ __forceinline__ void pg_adjoint_inv(const double* R, const double* t, double* Ad) {
  double Rt[9], tt[3];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) Rt[a * 3 + b] = R[b * 3 + a];
  m3_tvec(R, t, tt);
#pragma unroll
  for (int a = 0; a < 3; ++a) tt[a] = -tt[a];
  pg_adjoint(Rt, tt, Ad);
}
// inverse left Jacobian of SE(3) at xi = (rho, phi), closed form (Barfoot, State Estimation for Robotics, 7.85-7.86)
__device__ __forceinline__ void pg_jl_inv(const double* xi, double* J) {
  const double* rho = xi;
  const double* phi = xi + 3;
  const double x = (phi[0] * phi[0] + phi[1] * phi[1]) + phi[2] * phi[2];
  const PgCoef c = pg_coeffs(x);
  double P[9], F[9], FP[9], PF[9], FF[9], FPF[9], FFP[9], PFF[9], FPFF[9], FFPF[9], Q[9], Ji[9], T1[9], T2[9];
  m3_hat(rho, P);
  m3_hat(phi, F);
  m3_mul(F, P, FP);
  m3_mul(P, F, PF);
  m3_mul(F, F, FF);
  m3_mul(FP, F, FPF);
  m3_mul(F, FP, FFP);
  m3_mul(PF, F, PFF);
  m3_mul(FPF, F, FPFF);
  m3_mul(F, FPF, FFPF);
#pragma unroll
  for (int q = 0; q < 9; ++q) {
    Q[q] = ((0.5 * P[q] + c.c1 * ((FP[q] + PF[q]) + FPF[q])) + c.c2 * ((FFP[q] + PFF[q]) - 3.0 * FPF[q])) + c.c3 * (FPFF[q] + FFPF[q]);
    Ji[q] = (((q % 4 == 0) ? 1.0 : 0.0) - 0.5 * F[q]) + c.e * FF[q];
  }
  m3_mul(Ji, Q, T1);
  m3_mul(T1, Ji, T2);
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      J[i * 6 + j] = Ji[i * 3 + j];
      J[i * 6 + 3 + j] = -T2[i * 3 + j];
      J[(i + 3) * 6 + j] = 0.0;
      J[(i + 3) * 6 + 3 + j] = Ji[i * 3 + j];
    }
}
// inverse of a 6 x 6 SPD block by Cholesky; false (and `inv` untouched) on a non-positive or non-finite pivot
__device__ __forceinline__ bool pg_chol_inv(const double* D, double* inv) {
  double L[36], Li[36];
#pragma unroll
  for (int q = 0; q < 36; ++q) L[q] = Li[q] = 0.0;
  bool ok = true;
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    double d = D[c * 6 + c];
#pragma unroll
    for (int t = 0; t < c; ++t) d = d - L[c * 6 + t] * L[c * 6 + t];
    if (!(d > 0.0) || !(d * 0.0 == 0.0)) ok = false;
    const double l = sqrt(ok ? d : 1.0);
    L[c * 6 + c] = l;
#pragma unroll
    for (int r = c + 1; r < 6; ++r) {
      double v = D[r * 6 + c];
#pragma unroll
      for (int t = 0; t < c; ++t) v = v - L[r * 6 + t] * L[c * 6 + t];
      L[r * 6 + c] = v / l;
    }
  }
  if (!ok) return false;
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    Li[c * 6 + c] = 1.0 / L[c * 6 + c];
#pragma unroll
    for (int r = c + 1; r < 6; ++r) {
      double v = 0.0;
#pragma unroll
      for (int t = c; t < r; ++t) v = v - L[r * 6 + t] * Li[t * 6 + c];
      Li[r * 6 + c] = v / L[r * 6 + r];
    }
  }
  double out[36];
  m6_tmul(Li, Li, out);
  bool fin = true;
#pragma unroll
  for (int q = 0; q < 36; ++q) fin = fin && (out[q] * 0.0 == 0.0);
  if (!fin) return false;
#pragma unroll
  for (int q = 0; q < 36; ++q) inv[q] = out[q];
  return true;
}

// sum / maximum of one value per thread over the workgroup by a halving tree; the result is valid on thread 0
__device__ __forceinline__ double pg_wg_sum(double v, double* sh) {
  __syncthreads();
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int h = PG_B / 2; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) sh[threadIdx.x] = sh[threadIdx.x] + sh[threadIdx.x + h];
    __syncthreads();
  }
  return sh[0];
}
__device__ __forceinline__ double pg_wg_max(double v, double* sh) {
  __syncthreads();
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int h = PG_B / 2; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) sh[threadIdx.x] = fmax(sh[threadIdx.x], sh[threadIdx.x + h]);
    __syncthreads();
  }
  return sh[0];
}
// the same over n per-workgroup partials (stride `stride` doubles) inside ONE workgroup: lane t takes partials t, t + 256, ... in order
__device__ __forceinline__ double pg_partial_sum(const double* part, int n, int stride, double* sh) {
  double v = 0.0;
  for (int k = threadIdx.x; k < n; k += PG_B) v = v + part[(size_t)k * stride];
  return pg_wg_sum(v, sh);
}
__device__ __forceinline__ double pg_partial_max(const double* part, int n, int stride, double* sh) {
  double v = 0.0;
  for (int k = threadIdx.x; k < n; k += PG_B) v = fmax(v, part[(size_t)k * stride]);
  return pg_wg_max(v, sh);
}
__device__ __forceinline__ bool pg_stopped(const double* rec) { return rec != nullptr && (rec[R_CONV] != 0.0 || rec[R_BREAK] != 0.0); }

// ---- linearization ------------------------------------------------------------------------------------------------------------------------
// one edge per thread: r, s, w, rho; with JAC also A, B, the three Hessian blocks and the two gradient terms
template <bool JAC>
__global__ __launch_bounds__(PG_B) void pg_edge_kernel(const double* __restrict__ poses, int N, const int32_t* __restrict__ ij,
                                                       const double* __restrict__ meas, const double* __restrict__ info, int E,
                                                       double huber, double* __restrict__ res, double* __restrict__ chi,
                                                       double* __restrict__ weight, double* __restrict__ jac,
                                                       double* __restrict__ blocks, double* __restrict__ eg, double* __restrict__ part) {
  __shared__ double sh[PG_B];
  const int e = blockIdx.x * PG_B + threadIdx.x;
  double rho = 0.0, bad = 0.0;
  if (e < E) {
    const int i = ij[2 * e], j = ij[2 * e + 1];
    double r[6] = {0, 0, 0, 0, 0, 0}, s = 0.0, w = 0.0;
    double Om[36], A[36], B[36];
    bool ok = i >= 0 && i < N && j >= 0 && j < N && i != j;
    if (ok) {
      double Ri[9], ti[3], Rj[9], tj[3], Rz[9], tz[3], Rij[9], tij[3], Rd[9], td[3];
      pg_load_pose(poses + (size_t)i * 16, Ri, ti);
      pg_load_pose(poses + (size_t)j * 16, Rj, tj);
      pg_load_pose(meas + (size_t)e * 16, Rz, tz);
      ld36(info + (size_t)e * 36, Om);
      double f = 0.0;
#pragma unroll
      for (int q = 0; q < 36; ++q) f += Om[q] * 0.0;
      ok = pg_finite12(Ri, ti) && pg_finite12(Rj, tj) && pg_finite12(Rz, tz) && f == 0.0;
      if (ok) {
        pg_rel(Ri, ti, Rj, tj, Rij, tij);
        pg_rel(Rz, tz, Rij, tij, Rd, td);
        pg_log(Rd, td, r);
        ok = v6_dot(r, r) * 0.0 == 0.0;
      }
      if (ok) {
        double Or[6];
        m6_vec(Om, r, Or);
        const double s2 = v6_dot(r, Or);
        s = sqrt(s2 > 0.0 ? s2 : 0.0);
        if (s <= huber) {
          rho = (0.5 * s) * s;
          w = 1.0;
        } else {
          rho = huber * (s - 0.5 * huber);
          w = huber / s;
        }
        if (JAC) {
          const double nr[6] = {-r[0], -r[1], -r[2], -r[3], -r[4], -r[5]};
          pg_jl_inv(nr, B);                      // J_r^-1(r) = J_l^-1(-r)
          double Ad[36];
          pg_adjoint_inv(Rij, tij, Ad);          // Ad(T_ij^-1)
          m6_mul(B, Ad, A);
#pragma unroll
          for (int q = 0; q < 36; ++q) A[q] = -A[q];
          double g[6], t6[6];
          m6_tvec(A, Or, t6);
#pragma unroll
          for (int q = 0; q < 6; ++q) g[q] = w * t6[q];
          st6(eg + (size_t)e * 12, g);
          m6_tvec(B, Or, t6);
#pragma unroll
          for (int q = 0; q < 6; ++q) g[q] = w * t6[q];
          st6(eg + (size_t)e * 12 + 6, g);
        }
      }
    }
    if (!ok) {
      bad = 1.0;
      rho = 0.0;
      s = 0.0;
      w = 0.0;
#pragma unroll
      for (int q = 0; q < 6; ++q) r[q] = 0.0;
    }
    st6(res + (size_t)e * 6, r);
    chi[e] = s;
    weight[e] = w;
    if (JAC) {
      double* jb = jac + (size_t)e * 72;
      double* hb = blocks + (size_t)e * 108;
      if (ok) {
        double W6[36], H[36];
        st36(jb, A);
        st36(jb + 36, B);
        m6_mul(Om, B, W6);
#pragma unroll
        for (int q = 0; q < 36; ++q) W6[q] = w * W6[q];
        m6_tmul(B, W6, H);
        st36(hb + 72, H);
        m6_tmul(A, W6, H);
        st36(hb + 36, H);
        m6_mul(Om, A, W6);
#pragma unroll
        for (int q = 0; q < 36; ++q) W6[q] = w * W6[q];
        m6_tmul(A, W6, H);
        st36(hb, H);
      } else {
        for (int q = 0; q < 72; ++q) jb[q] = 0.0;
        for (int q = 0; q < 108; ++q) hb[q] = 0.0;
        for (int q = 0; q < 12; ++q) eg[(size_t)e * 12 + q] = 0.0;
      }
    }
  }
  const double c = pg_wg_sum(rho, sh);
  const double nb = pg_wg_sum(bad, sh);
  if (threadIdx.x == 0) {
    part[2 * blockIdx.x] = c;
    part[2 * blockIdx.x + 1] = nb;
  }
}

// one node per thread: gradient, diagonal block and its inverse over the incidence list, in list order
__global__ __launch_bounds__(PG_B) void pg_node_kernel(const uint8_t* __restrict__ fixed, int N, const int32_t* __restrict__ ij, int E,
                                                       const int32_t* __restrict__ ptr, const int32_t* __restrict__ lst,
                                                       const double* __restrict__ blocks, const double* __restrict__ eg,
                                                       double* __restrict__ grad, double* __restrict__ diag, double* __restrict__ dinv,
                                                       double* __restrict__ part) {
  __shared__ double sh[PG_B];
  const int v = blockIdx.x * PG_B + threadIdx.x;
  double fail = 0.0, gmax = 0.0;
  if (v < N) {
    double g[6], D[36], Di[36];
#pragma unroll
    for (int q = 0; q < 6; ++q) g[q] = 0.0;
#pragma unroll
    for (int q = 0; q < 36; ++q) D[q] = Di[q] = 0.0;
    if (!fixed[v]) {
      int b = ptr[v], en = ptr[v + 1];
      b = b < 0 ? 0 : b;
      en = en > 2 * E ? 2 * E : en;
      bool first = true;
      for (int k = b; k < en; ++k) {
        const int e = lst[k];
        if (e < 0 || e >= E) continue;
        const int side = ij[2 * e] == v ? 0 : 1;
        const double* gp = eg + (size_t)e * 12 + 6 * side;
        const double* hp = blocks + (size_t)e * 108 + 72 * side;
        if (first) {
#pragma unroll
          for (int q = 0; q < 6; ++q) g[q] = gp[q];
#pragma unroll
          for (int q = 0; q < 36; ++q) D[q] = hp[q];
          first = false;
        } else {
#pragma unroll
          for (int q = 0; q < 6; ++q) g[q] = g[q] + gp[q];
#pragma unroll
          for (int q = 0; q < 36; ++q) D[q] = D[q] + hp[q];
        }
      }
      if (!pg_chol_inv(D, Di)) fail = 1.0;
#pragma unroll
      for (int q = 0; q < 6; ++q) gmax = fmax(gmax, fabs(g[q]));
    }
    st6(grad + (size_t)v * 6, g);
    st36(diag + (size_t)v * 36, D);
    st36(dinv + (size_t)v * 36, Di);
  }
  const double f = pg_wg_sum(fail, sh);
  const double m = pg_wg_max(gmax, sh);
  if (threadIdx.x == 0) {
    part[2 * blockIdx.x] = f;
    part[2 * blockIdx.x + 1] = m;
  }
}

// one chain edge m = (m, m + 1) per thread: G_m = P (w Omega)^-1 P' with P = Ad(T_{m+1}) B_m^-1, and N_m = Ad(T_{m+1}^-1)
__global__ __launch_bounds__(PG_B) void pg_chain_kernel(const double* __restrict__ poses, int N, const double* __restrict__ info,
                                                        const double* __restrict__ weight, const double* __restrict__ jac,
                                                        double* __restrict__ chain, double* __restrict__ part) {
  __shared__ double sh[PG_B];
  const int m = blockIdx.x * PG_B + threadIdx.x;
  double fail = 0.0;
  if (m < N - 1) {
    double G[36], Nm[36];
#pragma unroll
    for (int q = 0; q < 36; ++q) G[q] = Nm[q] = 0.0;
    double R[9], t[3];
    pg_load_pose(poses + (size_t)(m + 1) * 16, R, t);
    const double* B = jac + (size_t)m * 72 + 36;
    double J[9], K[9], Ji[9];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = 0; b < 3; ++b) {
        J[a * 3 + b] = B[a * 6 + b];
        K[a * 3 + b] = B[a * 6 + 3 + b];
      }
    const double c00 = J[4] * J[8] - J[5] * J[7], c01 = J[5] * J[6] - J[3] * J[8], c02 = J[3] * J[7] - J[4] * J[6];
    const double det = (J[0] * c00 + J[1] * c01) + J[2] * c02;
    const double id = 1.0 / det;
    Ji[0] = c00 * id; Ji[1] = (J[2] * J[7] - J[1] * J[8]) * id; Ji[2] = (J[1] * J[5] - J[2] * J[4]) * id;
    Ji[3] = c01 * id; Ji[4] = (J[0] * J[8] - J[2] * J[6]) * id; Ji[5] = (J[2] * J[3] - J[0] * J[5]) * id;
    Ji[6] = c02 * id; Ji[7] = (J[1] * J[6] - J[0] * J[7]) * id; Ji[8] = (J[0] * J[4] - J[1] * J[3]) * id;
    double T1[9], T2[9], Binv[36], Ad[36], P[36], Wm[36], Wi[36], PW[36];
    m3_mul(Ji, K, T1);
    m3_mul(T1, Ji, T2);
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = 0; b < 3; ++b) {
        Binv[a * 6 + b] = Ji[a * 3 + b];
        Binv[a * 6 + 3 + b] = -T2[a * 3 + b];
        Binv[(a + 3) * 6 + b] = 0.0;
        Binv[(a + 3) * 6 + 3 + b] = Ji[a * 3 + b];
      }
    pg_adjoint(R, t, Ad);
    m6_mul(Ad, Binv, P);
    const double w = weight[m];
#pragma unroll
    for (int q = 0; q < 36; ++q) Wm[q] = w * info[(size_t)m * 36 + q];
    bool ok = pg_chol_inv(Wm, Wi);
    if (ok) {
      m6_mul(P, Wi, PW);
      m6_mult(PW, P, G);
      pg_adjoint_inv(R, t, Nm);
      double f = 0.0;
#pragma unroll
      for (int q = 0; q < 36; ++q) f += (G[q] + Nm[q]) * 0.0;
      ok = f == 0.0;
    }
    if (!ok) {
      fail = 1.0;
#pragma unroll
      for (int q = 0; q < 36; ++q) G[q] = Nm[q] = 0.0;
    }
    st36(chain + (size_t)m * 72, G);
    st36(chain + (size_t)m * 72 + 36, Nm);
  }
  const double f = pg_wg_sum(fail, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = f;
}

// ONE workgroup: the linearization's slots of the record
__global__ __launch_bounds__(PG_B) void pg_lin_record_kernel(const double* part_e, int nbe, const double* part_n, int nbn,
                                                             const double* part_c, int nbc, double* rec) {
  __shared__ double sh[PG_B];
  const double cost = pg_partial_sum(part_e, nbe, 2, sh);
  const double bad = pg_partial_sum(part_e + 1, nbe, 2, sh);
  double fail = 0.0, gmax = 0.0, cfail = 0.0;
  if (part_n) {
    fail = pg_partial_sum(part_n, nbn, 2, sh);
    gmax = pg_partial_max(part_n + 1, nbn, 2, sh);
  }
  if (part_c) cfail = pg_partial_sum(part_c, nbc, 1, sh);
  if (threadIdx.x == 0) {
    rec[R_COST] = cost;
    rec[R_BAD] = bad;
    rec[R_CHOL] = fail + cfail;
    rec[R_GMAX] = gmax;
  }
}

__global__ void pg_set_record_kernel(double* rec, int first, int n, double value) {
  const int k = threadIdx.x;
  if (k < n) rec[first + k] = value;
}

// ---- the solver ---------------------------------------------------------------------------------------------------------------------------
// the start of a solve: `breakdown` from the linearization's failed pivots and, with `loops`, the prepare's
__global__ void pg_solve_reset_kernel(double* rec, int loops) {
  if (threadIdx.x != 0) return;
  rec[R_ITER] = 0.0;
  rec[R_REL] = 1.0;
  rec[R_CONV] = 0.0;
  rec[R_BREAK] = (rec[R_CHOL] != 0.0 || (loops && rec[R_LPIV] != 0.0)) ? 1.0 : 0.0;
  rec[R_RZ] = rec[R_RZ0] = rec[R_ALPHA] = rec[R_BETA] = 0.0;
}

// z = Dinv r / (1 + lambda) of one node, and its term of r . z
__device__ __forceinline__ double pg_jacobi_node(const double* dinv, double scale, const double* r, double* z) {
  double Di[36], t6[6];
  ld36(dinv, Di);
  m6_vec(Di, r, t6);
#pragma unroll
  for (int q = 0; q < 6; ++q) z[q] = scale * t6[q];
  return v6_dot(r, z);
}

// x = 0, r = -g, both search directions 0; with `dinv` also z = M^-1 r (block-Jacobi) and the partials of r . z
__global__ __launch_bounds__(PG_B) void pg_solve_init_kernel(const uint8_t* __restrict__ fixed, int N, const double* __restrict__ grad,
                                                             const double* __restrict__ dinv, double scale, double* __restrict__ x,
                                                             double* __restrict__ r, double* __restrict__ z, double* __restrict__ p0,
                                                             double* __restrict__ p1, double* __restrict__ part, const double* rec) {
  if (pg_stopped(rec)) return;
  __shared__ double sh[PG_B];
  const int v = blockIdx.x * PG_B + threadIdx.x;
  double d = 0.0;
  if (v < N) {
    double rv[6], zv[6];
    const bool fx = fixed[v] != 0;
#pragma unroll
    for (int q = 0; q < 6; ++q) {
      rv[q] = fx ? 0.0 : -grad[(size_t)v * 6 + q];
      zv[q] = 0.0;
    }
    if (dinv) d = pg_jacobi_node(dinv + (size_t)v * 36, scale, rv, zv);
#pragma unroll
    for (int q = 0; q < 6; ++q) {
      x[(size_t)v * 6 + q] = 0.0;
      p0[(size_t)v * 6 + q] = 0.0;
      p1[(size_t)v * 6 + q] = 0.0;
    }
    st6(r + (size_t)v * 6, rv);
    st6(z + (size_t)v * 6, zv);
  }
  if (dinv) {
    const double s = pg_wg_sum(d, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
  }
}

// ONE workgroup: rz0 = rz = r . z of the start
__global__ __launch_bounds__(PG_B) void pg_solve_rz0_kernel(const double* part, int nb, double* rec) {
  if (pg_stopped(rec)) return;
  __shared__ double sh[PG_B];
  const double rz = pg_partial_sum(part, nb, 1, sh);
  if (threadIdx.x == 0) {
    rec[R_RZ] = rec[R_RZ0] = rz;
    rec[R_BETA] = 0.0;
    if (rz == 0.0) {
      rec[R_REL] = 0.0;
      rec[R_CONV] = 1.0;
    } else if (!(rz > 0.0) || !(rz * 0.0 == 0.0)) {
      rec[R_BREAK] = 1.0;
    }
  }
}

// p = z + beta p_old for the node and its neighbours, q = (H + lambda blockdiag H) p over the incidence list, partials of p . q
__global__ __launch_bounds__(PG_B) void pg_matvec_kernel(const uint8_t* __restrict__ fixed, int N, const int32_t* __restrict__ ij, int E,
                                                         const int32_t* __restrict__ ptr, const int32_t* __restrict__ lst,
                                                         const double* __restrict__ blocks, const double* __restrict__ diag, double lambda,
                                                         const double* __restrict__ z, const double* __restrict__ pold,
                                                         double* __restrict__ pnew, double* __restrict__ q, double* __restrict__ part,
                                                         const double* rec) {
  if (pg_stopped(rec)) return;
  __shared__ double sh[PG_B];
  const double beta = rec[R_BETA];
  const int v = blockIdx.x * PG_B + threadIdx.x;
  double d = 0.0;
  if (v < N) {
    double pv[6], acc[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) pv[k] = acc[k] = 0.0;
    if (!fixed[v]) {
#pragma unroll
      for (int k = 0; k < 6; ++k) pv[k] = z[(size_t)v * 6 + k] + beta * pold[(size_t)v * 6 + k];
      double M[36], t6[6], u6[6];
      ld36(diag + (size_t)v * 36, M);
      m6_vec(M, pv, t6);
#pragma unroll
      for (int k = 0; k < 6; ++k) acc[k] = lambda * t6[k];
      int b = ptr[v], en = ptr[v + 1];
      b = b < 0 ? 0 : b;
      en = en > 2 * E ? 2 * E : en;
      for (int c = b; c < en; ++c) {
        const int e = lst[c];
        if (e < 0 || e >= E) continue;
        const int i = ij[2 * e], j = ij[2 * e + 1];
        if (i < 0 || i >= N || j < 0 || j >= N || i == j) continue;
        double xi[6], xj[6];
        const bool fi = fixed[i] != 0, fj = fixed[j] != 0;
#pragma unroll
        for (int k = 0; k < 6; ++k) {
          xi[k] = fi ? 0.0 : z[(size_t)i * 6 + k] + beta * pold[(size_t)i * 6 + k];
          xj[k] = fj ? 0.0 : z[(size_t)j * 6 + k] + beta * pold[(size_t)j * 6 + k];
        }
        const double* hb = blocks + (size_t)e * 108;
        if (i == v) {
          ld36(hb, M);
          m6_vec(M, xi, t6);
          ld36(hb + 36, M);
          m6_vec(M, xj, u6);
        } else {
          ld36(hb + 36, M);
          m6_tvec(M, xi, t6);
          ld36(hb + 72, M);
          m6_vec(M, xj, u6);
        }
#pragma unroll
        for (int k = 0; k < 6; ++k) acc[k] = acc[k] + (t6[k] + u6[k]);
      }
      d = v6_dot(pv, acc);
    }
    st6(pnew + (size_t)v * 6, pv);
    st6(q + (size_t)v * 6, acc);
  }
  const double s = pg_wg_sum(d, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// ONE workgroup: alpha = rz / p . q, or breakdown
__global__ __launch_bounds__(PG_B) void pg_alpha_kernel(const double* part, int nb, double* rec) {
  if (pg_stopped(rec)) return;
  __shared__ double sh[PG_B];
  const double pq = pg_partial_sum(part, nb, 1, sh);
  if (threadIdx.x == 0) {
    const double a = rec[R_RZ] / pq;
    if (!(pq > 0.0) || !(a * 0.0 == 0.0)) rec[R_BREAK] = 1.0;
    else rec[R_ALPHA] = a;
  }
}

// x += alpha p, r -= alpha q; with `dinv` also z = M^-1 r (block-Jacobi) and the partials of r . z
__global__ __launch_bounds__(PG_B) void pg_update_kernel(int N, const double* __restrict__ p, const double* __restrict__ q,
                                                         const double* __restrict__ dinv, double scale, double* __restrict__ x,
                                                         double* __restrict__ r, double* __restrict__ z, double* __restrict__ part,
                                                         const double* rec) {
  if (pg_stopped(rec)) return;
  __shared__ double sh[PG_B];
  const double alpha = rec[R_ALPHA];
  const int v = blockIdx.x * PG_B + threadIdx.x;
  double d = 0.0;
  if (v < N) {
    double rv[6], zv[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      x[(size_t)v * 6 + k] = x[(size_t)v * 6 + k] + alpha * p[(size_t)v * 6 + k];
      rv[k] = r[(size_t)v * 6 + k] - alpha * q[(size_t)v * 6 + k];
    }
    st6(r + (size_t)v * 6, rv);
    if (dinv) {
      d = pg_jacobi_node(dinv + (size_t)v * 36, scale, rv, zv);
      st6(z + (size_t)v * 6, zv);
    }
  }
  if (dinv) {
    const double s = pg_wg_sum(d, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
  }
}

// ONE workgroup: beta = rz' / rz, the iteration count and the convergence test sqrt(rz' / rz0) <= rtol
__global__ __launch_bounds__(PG_B) void pg_beta_kernel(const double* part, int nb, double rtol, double* rec) {
  if (pg_stopped(rec)) return;
  __shared__ double sh[PG_B];
  const double rz = pg_partial_sum(part, nb, 1, sh);
  if (threadIdx.x == 0) {
    if (!(rz >= 0.0) || !(rz * 0.0 == 0.0)) {
      rec[R_BREAK] = 1.0;
      return;
    }
    const double rel = sqrt(rz / rec[R_RZ0]);
    rec[R_BETA] = rz / rec[R_RZ];
    rec[R_RZ] = rz;
    rec[R_ITER] = rec[R_ITER] + 1.0;
    rec[R_REL] = rel;
    if (rel <= rtol) rec[R_CONV] = 1.0;
  }
}

// ---- the scan: inclusive prefix sums of n 6-vectors (REV: from the last element down) in `rows` rows, three launches ----------------------
// Element l of the scan is element m = l (REV: n - 1 - l) of the data; block b holds the elements l = 256 b .. 256 b + 255.
// The block-local Hillis-Steele scan of one 6-vector per thread; the result is sh[returned][threadIdx.x]
__device__ __forceinline__ int pg_block_scan6(double (*sh)[PG_B][6], const double* v) {
  int cur = 0;
  st6(sh[0][threadIdx.x], v);
  __syncthreads();
  for (int d = 1; d < PG_B; d <<= 1) {
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      const double a = sh[cur][threadIdx.x][k];
      sh[cur ^ 1][threadIdx.x][k] = (int)threadIdx.x >= d ? a + sh[cur][threadIdx.x - d][k] : a;
    }
    cur ^= 1;
    __syncthreads();
  }
  return cur;
}

// launch 1, grid (blocks, rows): load(m, row, v) gives element m of a row (v arrives as zeros); the block-local scan goes to
// local[m * stride + 6 row], the block's total (written by its last live thread) to bsum
template <bool REV, class Load>
__global__ __launch_bounds__(PG_B) void pg_scan_local_kernel(int n, Load load, double* __restrict__ local, int stride,
                                                             double* __restrict__ bsum, const double* rec) {
  if (pg_stopped(rec)) return;
  __shared__ double sh[2][PG_B][6];
  const int l = blockIdx.x * PG_B + threadIdx.x, row = blockIdx.y;
  const int m = REV ? n - 1 - l : l;
  double v[6] = {0, 0, 0, 0, 0, 0};
  if (l < n) load(m, row, v);
  const int cur = pg_block_scan6(sh, v);
  if (l < n) st6(local + (size_t)m * stride + row * 6, sh[cur][threadIdx.x]);
  const int last = min(n - (int)blockIdx.x * PG_B, PG_B) - 1;
  if ((int)threadIdx.x == last) st6(bsum + ((size_t)row * gridDim.x + blockIdx.x) * 6, sh[cur][threadIdx.x]);
}
// the loaders.  A plain row: in[m]
struct PgLoadRow {
  const double* in;
  __device__ __forceinline__ void operator()(int m, int, double* v) const { ld6(in + (size_t)m * 6, v); }
};
// N_m' in[m + 1] (`in` has a row per NODE)
struct PgLoadNt {
  const double *in, *chain;
  __device__ __forceinline__ void operator()(int m, int, double* v) const {
    double Nm[36], y[6];
    ld36(chain + (size_t)m * 72 + 36, Nm);
    ld6(in + (size_t)(m + 1) * 6, y);
    m6_tvec(Nm, y, v);
  }
};
// row `row` of the 6 x 6 block G_m
struct PgLoadG {
  const double* chain;
  __device__ __forceinline__ void operator()(int m, int row, double* v) const { ld6(chain + (size_t)m * 72 + row * 6, v); }
};
// chain edge m takes + sigma_a C_a' d_a for the loop edges whose lo is node m and - for those whose hi is node m, over node m's
// incidence list in list order
struct PgLoadLoopDiff {
  int N, E, L;
  const int32_t *ptr, *lst;
  const double *C, *span, *d;
  __device__ __forceinline__ void operator()(int m, int, double* v) const {
    int b = ptr[m], en = ptr[m + 1];
    b = b < 0 ? 0 : b;
    en = en > 2 * E ? 2 * E : en;
    for (int k = b; k < en; ++k) {
      const int a = lst[k] - (N - 1);
      if (a < 0 || a >= L || span[4 * a + 3] == 0.0) continue;
      double Ca[36], da[6], t6[6];
      ld36(C + (size_t)a * 36, Ca);
      ld6(d + (size_t)a * 6, da);
      m6_tvec(Ca, da, t6);
      const double sg = span[4 * a + 2];
      if ((int)span[4 * a] == m) {
#pragma unroll
        for (int q = 0; q < 6; ++q) v[q] = v[q] + sg * t6[q];
      } else if ((int)span[4 * a + 1] == m) {
#pragma unroll
        for (int q = 0; q < 6; ++q) v[q] = v[q] - sg * t6[q];
      }
    }
  }
};

// launch 2, ONE workgroup, one lane per component: off[b] = the totals of the blocks before b, added in block order
__global__ void pg_scan_sums_kernel(int nb, int rows, const double* __restrict__ bsum, double* __restrict__ off, const double* rec) {
  if (pg_stopped(rec)) return;
  const int k = threadIdx.x;
  if (k >= 6 * rows) return;
  const int row = k / 6, q = k % 6;
  double tot = 0.0;
  for (int b = 0; b < nb; ++b) {
    const size_t at = ((size_t)row * nb + b) * 6 + q;
    off[at] = tot;
    tot = b ? tot + bsum[at] : bsum[at];
  }
}

// an element after launch 2: its block-local value and, past the first block, its block's offset
__device__ __forceinline__ void pg_scan_read(const double* loc, const double* off, bool first_block, double* c) {
  ld6(loc, c);
  if (!first_block) {
#pragma unroll
    for (int k = 0; k < 6; ++k) c[k] = c[k] + off[k];
  }
}
// c[m] of a forward scan of one row whose launch 3 has not run
__device__ __forceinline__ void pgl_prefix_at(const double* local, const double* off, int m, double* c) {
  pg_scan_read(local + (size_t)m * 6, off + (size_t)(m / PG_B) * 6, m < PG_B, c);
}

// launch 3, grid (blocks, rows): fin(m, row, first, v) finishes element m from its scanned value v (`first`: it is in the first
// block, whose values have no offset; a finisher that works IN_PLACE on `local` gets no v there) and returns its term of the dot
// product, summed per workgroup into fin.part where the finisher has one (Fin::DOT) and it is given.  The finishers' members cannot
// say that they do not alias: each passes them to a `run` whose parameters can, as the kernels' parameters do
template <bool REV, class Fin>
__global__ __launch_bounds__(PG_B) void pg_scan_apply_kernel(int n, const double* local, int stride, const double* __restrict__ off, Fin fin,
                                                             const double* rec) {
  if (pg_stopped(rec)) return;
  const int l = blockIdx.x * PG_B + threadIdx.x, row = blockIdx.y;
  const int m = REV ? n - 1 - l : l;
  double d = 0.0;
  if (l < n) {
    const bool first = blockIdx.x == 0;
    double v[6] = {0, 0, 0, 0, 0, 0};
    if (!(Fin::IN_PLACE && first))
      pg_scan_read(local + (size_t)m * stride + row * 6, off + ((size_t)row * gridDim.x + blockIdx.x) * 6, first, v);
    d = fin(m, row, first, v);
  }
  if constexpr (Fin::DOT) {
    if (fin.part) {
      __shared__ double sh[PG_B];
      const double s = pg_wg_sum(d, sh);
      if (threadIdx.x == 0) fin.part[blockIdx.x] = s;
    }
  }
}
// the finishers.  out[m] = G_m v, a row per chain edge; v itself is kept in keep[m] when `keep` is given
struct PgFinG {
  static constexpr bool DOT = false, IN_PLACE = false;
  const double* chain;
  double *keep, *out;
  static __device__ __forceinline__ void run(const double* __restrict__ chain, double* __restrict__ keep, double* __restrict__ out, int m,
                                             const double* v) {
    double M[36], o[6];
    if (keep) st6(keep + (size_t)m * 6, v);
    ld36(chain + (size_t)m * 72, M);
    m6_vec(M, v, o);
    st6(out + (size_t)m * 6, o);
  }
  __device__ __forceinline__ double operator()(int m, int, bool, const double* v) const {
    run(chain, keep, out, m, v);
    return 0.0;
  }
};
// out[m] = G_m (s[m] - v)
struct PgFinDiffG {
  static constexpr bool DOT = false, IN_PLACE = false;
  const double *chain, *s;
  double* out;
  __device__ __forceinline__ double operator()(int m, int, bool, const double* v) const {
    double sv[6], M[36], o[6];
    ld6(s + (size_t)m * 6, sv);
#pragma unroll
    for (int k = 0; k < 6; ++k) sv[k] = sv[k] - v[k];
    ld36(chain + (size_t)m * 72, M);
    m6_vec(M, sv, o);
    st6(out + (size_t)m * 6, o);
    return 0.0;
  }
};
// out[m + 1] = N_m v, a row per node, and its term of r . z when `r` is given
struct PgFinN {
  static constexpr bool DOT = true, IN_PLACE = false;
  const double* chain;
  double* out;
  const double* r;
  double* part;
  static __device__ __forceinline__ double run(const double* __restrict__ chain, double* __restrict__ out, const double* __restrict__ r,
                                               int m, const double* v) {
    double M[36], o[6];
    ld36(chain + (size_t)m * 72 + 36, M);
    m6_vec(M, v, o);
    st6(out + (size_t)(m + 1) * 6, o);
    if (!r) return 0.0;
    double rv[6];
    ld6(r + (size_t)(m + 1) * 6, rv);
    return v6_dot(rv, o);
  }
  __device__ __forceinline__ double operator()(int m, int, bool, const double* v) const { return run(chain, out, r, m, v); }
};
// Gamma in place: the block-local scan sits in Gamma[m + 1] already, so only the blocks past the first are written; Gamma[0] = 0
struct PgFinGamma {
  static constexpr bool DOT = false, IN_PLACE = true;
  double* gamma;
  __device__ __forceinline__ double operator()(int m, int row, bool first, const double* v) const {
    if (m == 0) {
#pragma unroll
      for (int k = 0; k < 6; ++k) gamma[row * 6 + k] = 0.0;
    }
    if (!first) st6(gamma + (size_t)(m + 1) * 36 + row * 6, v);
    return 0.0;
  }
};

// launches 1 and 2 of one scan; the offsets follow the block totals in `bsum` (12 * rows * blocks doubles)
template <bool REV, class Load>
void pg_scan_launch12(int n, int rows, Load load, double* local, int stride, double* bsum, const double* rec, hipStream_t stream) {
  const int nb = (n + PG_B - 1) / PG_B;
  pg_scan_local_kernel<REV><<<dim3(nb, rows), PG_B, 0, stream>>>(n, load, local, stride, bsum, rec);
  pg_scan_sums_kernel<<<1, 64, 0, stream>>>(nb, rows, bsum, bsum + (size_t)6 * rows * nb, rec);
}
// Gamma[k] = sum_{m < k} G_m, (n + 1, 6, 6), as six rows of six
void pg_gamma_scan(int n, const double* chain, double* gamma, double* gsum, hipStream_t stream) {
  const int nb = (n + PG_B - 1) / PG_B;
  pg_scan_launch12<false>(n, 6, PgLoadG{chain}, gamma + 36, 36, gsum, nullptr, stream);
  pg_scan_apply_kernel<false><<<dim3(nb, 6), PG_B, 0, stream>>>(n, gamma + 36, 36, gsum + (size_t)36 * nb, PgFinGamma{gamma}, nullptr);
}

// z = Dinv r / (1 + lambda) alone (ovn_pose_graph_precondition)
__global__ __launch_bounds__(PG_B) void pg_jacobi_apply_kernel(int N, const double* __restrict__ dinv, double scale,
                                                               const double* __restrict__ in, double* __restrict__ out) {
  const int v = blockIdx.x * PG_B + threadIdx.x;
  if (v >= N) return;
  double rv[6], zv[6];
  ld6(in + (size_t)v * 6, rv);
  (void)pg_jacobi_node(dinv + (size_t)v * 36, scale, rv, zv);
  st6(out + (size_t)v * 6, zv);
}

// ---- retraction ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PG_B) void pg_retract_kernel(const double* __restrict__ poses, const uint8_t* __restrict__ fixed,
                                                          const double* __restrict__ delta, int N, double* __restrict__ out,
                                                          double* __restrict__ part) {
  __shared__ double sh[PG_B];
  const int v = blockIdx.x * PG_B + threadIdx.x;
  double dm = 0.0;
  if (v < N) {
    double T[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) T[q] = poses[(size_t)v * 16 + q];
    if (!fixed[v]) {
      double R[9], t[3], xi[6], Re[9], te[3], Ro[9], to[3];
      pg_load_pose(T, R, t);
      ld6(delta + (size_t)v * 6, xi);
#pragma unroll
      for (int q = 0; q < 6; ++q) dm = fmax(dm, fabs(xi[q]));
      pg_exp(xi, Re, te);
      m3_mul(R, Re, Ro);
      m3_vec(R, te, to);
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        T[i * 4] = Ro[i * 3]; T[i * 4 + 1] = Ro[i * 3 + 1]; T[i * 4 + 2] = Ro[i * 3 + 2];
        T[i * 4 + 3] = to[i] + t[i];
      }
      T[12] = 0.0; T[13] = 0.0; T[14] = 0.0; T[15] = 1.0;
    }
#pragma unroll
    for (int q = 0; q < 16; ++q) out[(size_t)v * 16 + q] = T[q];
  }
  const double m = pg_wg_max(dm, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = m;
}

__global__ __launch_bounds__(PG_B) void pg_dmax_kernel(const double* part, int nb, double* rec) {
  __shared__ double sh[PG_B];
  const double m = pg_partial_max(part, nb, 1, sh);
  if (threadIdx.x == 0) rec[R_DMAX] = m;
}

bool pg_finite(double v) { return v * 0.0 == 0.0; }

// ---- the chain-plus-loops inverse (ovn_pose_graph_loops_*) -----------------------------------------------------------
// H = H_chain + sum_a J_a' w_a Omega_a J_a over the L loop edges; in chain coordinates J_a is sigma_a C_a times a sum over the chain
// edges [lo_a, hi_a), so Woodbury needs the 6 L x 6 L matrix S = W^-1 + J H_chain^-1 J', whose blocks are differences of the prefix
// sums Gamma of G.  S is factored by a blocked right-looking Cholesky (block PGL_NB) and applied by two triangular sweeps.
constexpr int PGL_NB = 48;                                  // block size of the factorization: eight 6 x 6 blocks
constexpr int PGL_TS = 1024;                                // threads of the one-workgroup triangular sweeps
constexpr int PGL_MAX_SP = (6 * OVN_POSE_GRAPH_MAX_LOOPS + PGL_NB - 1) / PGL_NB * PGL_NB;

struct PgLoops {   // the caller's loops_dev, in doubles
  double *gamma, *gsum, *C, *winv, *span, *s, *d, *part, *pf, *S, *F;
  int64_t sp, nbk, nbc, nbl;
  size_t total;
  PgLoops(double* base, int64_t N, int64_t L) {
    nbc = (N - 1 + PG_B - 1) / PG_B;
    nbl = (L + PG_B - 1) / PG_B;
    sp = (6 * L + PGL_NB - 1) / PGL_NB * PGL_NB;
    nbk = sp / PGL_NB;
    PgTake take{base};
    gamma = take(36 * N);       // Gamma[k] = sum_{m < k} G_m
    C = take(36 * L);           // C_a = B_a Ad(T_j^-1), 0 for an edge that is left out
    winv = take(36 * L);        // (w_a Omega_a)^-1, the identity for an edge that is left out
    span = take(4 * L);         // lo, hi, sigma, live
    S = take((size_t)sp * sp);
    F = take((size_t)sp * sp);  // the lower Cholesky factor of S, zero above the diagonal
    gsum = take(72 * nbc);      // the scan's block totals and offsets
    s = take(6 * N);
    d = take(sp);
    part = take(2 * nbl);
    pf = take(nbk);
    total = take.o;
  }
};

// the 48 x 48 block whose first entry is `a`, rows `lda` doubles apart, staged into LDS by the T threads of the workgroup; a second
// block (TWO) goes along in the same pass, so that both loads of an entry are in flight together
template <int T, bool TWO = false>
__device__ __forceinline__ void pgl_stage_tile(double (*A)[PGL_NB + 1], const double* a, size_t lda, double (*B)[PGL_NB + 1] = nullptr,
                                               const double* b = nullptr, size_t ldb = 0) {
  for (int t = threadIdx.x; t < PGL_NB * PGL_NB; t += T) {
    const int r = t / PGL_NB, c = t % PGL_NB;
    A[r][c] = a[(size_t)r * lda + c];
    if (TWO) B[r][c] = b[(size_t)r * ldb + c];
  }
}
// 3 x 3 entries per thread of the product of two staged tiles: acc[u][v] = sum_t A[tr + u][t] B[t][tc + v] (BT: B[tc + v][t]); the
// first term initialises, the rest are added in the order of t
template <bool BT>
__device__ __forceinline__ void pgl_tile_mul3(const double (*A)[PGL_NB + 1], const double (*B)[PGL_NB + 1], int tr, int tc,
                                              double (*acc)[3]) {
#pragma unroll
  for (int u = 0; u < 3; ++u)
#pragma unroll
    for (int v = 0; v < 3; ++v) acc[u][v] = A[tr + u][0] * (BT ? B[tc + v][0] : B[0][tc + v]);
#pragma unroll 4
  for (int t = 1; t < PGL_NB; ++t) {
    double av[3], bv[3];
#pragma unroll
    for (int u = 0; u < 3; ++u) {
      av[u] = A[tr + u][t];
      bv[u] = BT ? B[tc + u][t] : B[t][tc + u];
    }
#pragma unroll
    for (int u = 0; u < 3; ++u)
#pragma unroll
      for (int v = 0; v < 3; ++v) acc[u][v] = acc[u][v] + av[u] * bv[v];
  }
}

// one loop edge a = edge N - 1 + a per thread: C_a = B_a Ad(T_j^-1), (w_a Omega_a)^-1, lo, hi, sigma.  An edge of weight 0 is left out
// (zero C, identity block) and counted; an edge whose w Omega has no Cholesky factor is left out too and counted as a failed pivot
__global__ __launch_bounds__(PG_B) void pgl_edge_kernel(const double* __restrict__ poses, int N, const int32_t* __restrict__ ij,
                                                        const double* __restrict__ info, const double* __restrict__ weight,
                                                        const double* __restrict__ jac, int L, double* __restrict__ C,
                                                        double* __restrict__ winv, double* __restrict__ span, double* __restrict__ part) {
  __shared__ double sh[PG_B];
  const int a = blockIdx.x * PG_B + threadIdx.x;
  double fail = 0.0, out = 0.0;
  if (a < L) {
    const size_t e = (size_t)(N - 1) + a;
    const int i = ij[2 * e], j = ij[2 * e + 1];
    const double w = weight[e];
    bool live = w > 0.0 && i >= 0 && i < N && j >= 0 && j < N && i != j;
    double Ca[36], Wi[36];
#pragma unroll
    for (int q = 0; q < 36; ++q) {
      Ca[q] = 0.0;
      Wi[q] = (q % 7 == 0) ? 1.0 : 0.0;
    }
    if (!live) out = 1.0;
    if (live) {
      double Wm[36];
#pragma unroll
      for (int q = 0; q < 36; ++q) Wm[q] = w * info[e * 36 + q];
      if (!pg_chol_inv(Wm, Wi)) {
        fail = 1.0;
        live = false;
      }
    }
    if (live) {
      double R[9], t[3], Ad[36], Bm[36];
      pg_load_pose(poses + (size_t)j * 16, R, t);
      pg_adjoint_inv(R, t, Ad);
      ld36(jac + e * 72 + 36, Bm);
      m6_mul(Bm, Ad, Ca);
    }
    st36(C + (size_t)a * 36, Ca);
    st36(winv + (size_t)a * 36, Wi);
    span[4 * a] = live ? (double)min(i, j) : 0.0;
    span[4 * a + 1] = live ? (double)max(i, j) : 0.0;
    span[4 * a + 2] = live ? (j > i ? 1.0 : -1.0) : 0.0;
    span[4 * a + 3] = live ? 1.0 : 0.0;
  }
  const double f = pg_wg_sum(fail, sh);
  const double o = pg_wg_sum(out, sh);
  if (threadIdx.x == 0) {
    part[2 * blockIdx.x] = f;
    part[2 * blockIdx.x + 1] = o;
  }
}

// one 6 x 6 block (a, b), a <= b, per thread, written to (a, b) and transposed to (b, a):
// S_ab = delta_ab (w_a Omega_a)^-1 + sigma_a sigma_b (C_a (Gamma[min hi] - Gamma[max lo])) C_b' where the spans overlap.
// F gets the lower triangle of the same values and zeros above the diagonal.
__global__ __launch_bounds__(PG_B) void pgl_assemble_kernel(int L, int sp, const double* __restrict__ gamma, const double* __restrict__ C,
                                                            const double* __restrict__ winv, const double* __restrict__ span,
                                                            double* __restrict__ S, double* __restrict__ F) {
  const int a = blockIdx.y, b = blockIdx.x * PG_B + threadIdx.x;
  if (b >= L || b < a) return;
  double out[36];
#pragma unroll
  for (int q = 0; q < 36; ++q) out[q] = 0.0;
  if (span[4 * a + 3] != 0.0 && span[4 * b + 3] != 0.0) {
    const int lo = (int)fmax(span[4 * a], span[4 * b]), hi = (int)fmin(span[4 * a + 1], span[4 * b + 1]);
    if (lo < hi) {
      double M[36], T[36];
      const double* gh = gamma + (size_t)hi * 36;
      const double* gl = gamma + (size_t)lo * 36;
#pragma unroll
      for (int q = 0; q < 36; ++q) M[q] = gh[q] - gl[q];
      m6_mul(C + (size_t)a * 36, M, T);
      m6_mult(T, C + (size_t)b * 36, out);
      const double sg = span[4 * a + 2] * span[4 * b + 2];
#pragma unroll
      for (int q = 0; q < 36; ++q) out[q] = sg * out[q];
    }
  }
  if (a == b) {
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int j = i + 1; j < 6; ++j) out[i * 6 + j] = out[j * 6 + i];
#pragma unroll
    for (int q = 0; q < 36; ++q) out[q] = winv[(size_t)a * 36 + q] + out[q];
  }
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      const size_t up = (size_t)(6 * a + i) * sp + 6 * b + j, low = (size_t)(6 * b + j) * sp + 6 * a + i;
      const double v = out[i * 6 + j];
      S[up] = v;
      S[low] = v;
      if (a != b) {
        F[up] = 0.0;
        F[low] = v;
      } else {
        F[up] = i >= j ? v : 0.0;
      }
    }
}
// the padding rows and columns 6 L .. sp - 1: an identity diagonal
__global__ __launch_bounds__(PG_B) void pgl_pad_kernel(int n6, int sp, double* __restrict__ S, double* __restrict__ F) {
  const int64_t t = (int64_t)blockIdx.x * PG_B + threadIdx.x;
  if (t >= (int64_t)(sp - n6) * sp) return;
  const int row = n6 + (int)(t / sp), c = (int)(t % sp);
  const double v = c == row ? 1.0 : 0.0;
  S[(size_t)row * sp + c] = v;
  S[(size_t)c * sp + row] = v;
  F[(size_t)row * sp + c] = v;
  F[(size_t)c * sp + row] = v;
}

// the factorization, stage 1 of block column k, ONE wave: the Cholesky factor of the diagonal block, column by column as pg_chol_inv
// takes it (d = A_cc - sum_{t<c} L_ct^2 and v = A_rc - sum_{t<c} L_rt L_ct in the order of t, L_rc = v / sqrt d).  A pivot that is not
// positive and finite is counted in pf[k] and replaced by 1
__global__ __launch_bounds__(64) void pgl_panel_kernel(int sp, int k, double* __restrict__ F, double* __restrict__ pf) {
  __shared__ double A[PGL_NB][PGL_NB + 1];
  const int lane = threadIdx.x;
  const size_t base = (size_t)k * PGL_NB;
  pgl_stage_tile<64>(A, F + base * sp + base, sp);
  __syncthreads();
  double fails = 0.0;
  for (int c = 0; c < PGL_NB; ++c) {
    double d = A[c][c];
    for (int t = 0; t < c; ++t) d = d - A[c][t] * A[c][t];
    const bool ok = d > 0.0 && d * 0.0 == 0.0;
    if (!ok) fails += 1.0;
    const double l = sqrt(ok ? d : 1.0);
    double v = 0.0;
    if (lane > c && lane < PGL_NB) {
      v = A[lane][c];
      for (int t = 0; t < c; ++t) v = v - A[lane][t] * A[c][t];
      v = v / l;
    }
    __syncthreads();
    if (lane > c && lane < PGL_NB) A[lane][c] = v;
    if (lane == c) A[c][c] = l;
    __syncthreads();
  }
  for (int t = lane; t < PGL_NB * PGL_NB; t += 64) {
    const int r = t / PGL_NB, c = t % PGL_NB;
    if (r >= c) F[(base + r) * sp + base + c] = A[r][c];
  }
  if (lane == 0) pf[k] = fails;
}
// stage 2, one row below the diagonal block per thread: L_rk = A_rk L_kk^-T by forward substitution in column order
__global__ __launch_bounds__(PG_B) void pgl_trsm_kernel(int sp, int k, double* __restrict__ F) {
  __shared__ double Lk[PGL_NB][PGL_NB + 1];
  const size_t base = (size_t)k * PGL_NB;
  pgl_stage_tile<PG_B>(Lk, F + base * sp + base, sp);
  __syncthreads();
  const size_t r = base + PGL_NB + (size_t)blockIdx.x * PG_B + threadIdx.x;
  if (r >= (size_t)sp) return;
  double* p = F + r * sp + base;
  double x[PGL_NB];
#pragma unroll
  for (int c = 0; c < PGL_NB; ++c) {
    double v = p[c];
#pragma unroll
    for (int t = 0; t < c; ++t) v = v - x[t] * Lk[c][t];
    x[c] = v / Lk[c][c];
  }
#pragma unroll
  for (int c = 0; c < PGL_NB; ++c) p[c] = x[c];
}
// stage 3, one 48 x 48 tile (ti >= tj) of the trailing matrix per workgroup, 3 x 3 entries per thread:
// A_rc <- A_rc - (sum_t L_rt L_ct), the sum in the order of t, then one subtraction
__global__ __launch_bounds__(PG_B) void pgl_syrk_kernel(int sp, int k, double* __restrict__ F) {
  const int ti = blockIdx.y, tj = blockIdx.x;
  if (tj > ti) return;
  __shared__ double A[PGL_NB][PGL_NB + 1], B[PGL_NB][PGL_NB + 1];
  const size_t p0 = (size_t)k * PGL_NB, r0 = p0 + (size_t)(1 + ti) * PGL_NB, c0 = p0 + (size_t)(1 + tj) * PGL_NB;
  pgl_stage_tile<PG_B, true>(A, F + r0 * sp + p0, sp, B, F + c0 * sp + p0, sp);
  __syncthreads();
  const int tr = threadIdx.x / 16 * 3, tc = threadIdx.x % 16 * 3;
  double acc[3][3];
  pgl_tile_mul3<true>(A, B, tr, tc, acc);
#pragma unroll
  for (int u = 0; u < 3; ++u)
#pragma unroll
    for (int v = 0; v < 3; ++v) {
      if (ti == tj && tc + v > tr + u) continue;
      double* q = F + (r0 + tr + u) * sp + c0 + tc + v;
      *q = *q - acc[u][v];
    }
}
// ONE thread: record [13] and [14], every sum in index order
__global__ void pgl_record_kernel(const double* part, int nbl, const double* pf, int nbk, double* rec) {
  if (threadIdx.x != 0) return;
  double fail = 0.0, out = 0.0;
  for (int b = 0; b < nbl; ++b) {
    fail = fail + part[2 * b];
    out = out + part[2 * b + 1];
  }
  for (int k = 0; k < nbk; ++k) fail = fail + pf[k];
  rec[R_LPIV] = fail;
  rec[R_LOUT] = out;
}

// ONE workgroup: v_a = sigma_a C_a (c[hi_a - 1] - c[lo_a - 1]), then d = S^-1 v by L y = v and L' d = y.  Block column by block
// column: the diagonal block is solved in one wave (one subtraction per column, in column order: forward ascending, backward
// descending), then every remaining entry takes ONE subtraction of a 48-term sum in index order.  One launch: per block column a
// launch of its own measured slower up to 6 L = 1536 (profiles/pose_graph_loops.json)
__global__ __launch_bounds__(PGL_TS) void pgl_solve_kernel(int L, int sp, const double* __restrict__ local, const double* __restrict__ off,
                                                           const double* __restrict__ C, const double* __restrict__ span,
                                                           const double* __restrict__ F, double* __restrict__ d, const double* rec) {
  if (pg_stopped(rec)) return;
  __shared__ double x[PGL_MAX_SP];
  __shared__ double D[PGL_NB][PGL_NB + 1];
  const int tid = threadIdx.x;
  for (int idx = tid; idx < sp; idx += PGL_TS) {
    double v = 0.0;
    const int a = idx / 6, q = idx % 6;
    if (a < L && span[4 * a + 3] != 0.0) {
      const int lo = (int)span[4 * a], hi = (int)span[4 * a + 1];
      double ch[6], cl[6] = {0, 0, 0, 0, 0, 0};
      pgl_prefix_at(local, off, hi - 1, ch);
      if (lo > 0) pgl_prefix_at(local, off, lo - 1, cl);
      const double* cr = C + (size_t)a * 36 + q * 6;
      double s = cr[0] * (ch[0] - cl[0]);
#pragma unroll
      for (int k = 1; k < 6; ++k) s = s + cr[k] * (ch[k] - cl[k]);
      v = span[4 * a + 2] * s;
    }
    x[idx] = v;
  }
  __syncthreads();
  const int nbk = sp / PGL_NB;
  for (int k = 0; k < nbk; ++k) {
    const size_t base = (size_t)k * PGL_NB;
    pgl_stage_tile<PGL_TS>(D, F + base * sp + base, sp);
    __syncthreads();
    if (tid < 64) {
      double xv = tid < PGL_NB ? x[base + tid] : 0.0;
      for (int c = 0; c < PGL_NB; ++c) {
        const double y = __shfl(xv, c) / D[c][c];
        if (tid == c) xv = y;
        else if (tid > c && tid < PGL_NB) xv = xv - D[tid][c] * y;
      }
      if (tid < PGL_NB) x[base + tid] = xv;
    }
    __syncthreads();
    for (size_t r = base + PGL_NB + tid; r < (size_t)sp; r += PGL_TS) {
      const double* p = F + r * sp + base;
      double s = p[0] * x[base];
#pragma unroll 8
      for (int c = 1; c < PGL_NB; ++c) s = s + p[c] * x[base + c];
      x[r] = x[r] - s;
    }
    __syncthreads();
  }
  for (int k = nbk - 1; k >= 0; --k) {
    const size_t base = (size_t)k * PGL_NB;
    pgl_stage_tile<PGL_TS>(D, F + base * sp + base, sp);
    __syncthreads();
    if (tid < 64) {
      double xv = tid < PGL_NB ? x[base + tid] : 0.0;
      for (int c = PGL_NB - 1; c >= 0; --c) {
        const double y = __shfl(xv, c) / D[c][c];
        if (tid == c) xv = y;
        else if (tid < c) xv = xv - D[c][tid] * y;
      }
      if (tid < PGL_NB) x[base + tid] = xv;
    }
    __syncthreads();
    for (size_t r = tid; r < base; r += PGL_TS) {
      const double* p = F + base * sp + r;
      double s = p[0] * x[base];
#pragma unroll 8
      for (int c = 1; c < PGL_NB; ++c) s = s + p[(size_t)c * sp] * x[base + c];
      x[r] = x[r] - s;
    }
    __syncthreads();
  }
  for (int idx = tid; idx < sp; idx += PGL_TS) d[idx] = x[idx];
}

// ---- the preconditioners and the PCG loop they sit in ---------------------------------------------------------------------------------
struct PgPrecond {        // what a solve applies as M^-1
  const double* dj;       // block-Jacobi: dinv, applied inside the init and update kernels with `scale` = 1 / (1 + lambda); else NULL
  double scale;
  const double* chain;    // the chain (z = N S G S' N' r, S = inclusive prefix sums over the chain edges) and the loops; else NULL
  const PgLoops* lp;      // the chain-plus-loops inverse of L loop edges; else NULL
  int L;
};

// out = M^-1 in over the nodes 1 .. N - 1 (row 0 of `out` is not written: it is 0 from the start of a solve).  The chain alone is six
// launches; with loops the suffix scan s is kept, and between the two forward scans S^-1 is applied and the loop edges' terms are
// scanned and taken off s (out = H^-1 in, undamped): twelve launches
int pg_precond_apply(int N, int E, const int32_t* ptr, const int32_t* lst, const PgPrecond& pc, const double* in, double* out,
                     const PgWs& w, const double* r_for_dot, double* part, const double* rec, hipStream_t stream) {
  const int n = N - 1;
  if (n < 1) return OVN_OK;
  const int nb = (n + PG_B - 1) / PG_B;
  const double* chain = pc.chain;
  double* off = w.bsum + (size_t)6 * nb;
  pg_scan_launch12<true>(n, 1, PgLoadNt{in, chain}, w.sa, 6, w.bsum, rec, stream);
  pg_scan_apply_kernel<true><<<nb, PG_B, 0, stream>>>(n, w.sa, 6, off, PgFinG{chain, pc.lp ? pc.lp->s : nullptr, w.sb}, rec);
  pg_scan_launch12<false>(n, 1, PgLoadRow{w.sb}, w.sa, 6, w.bsum, rec, stream);
  if (pc.lp) {
    const PgLoops& lp = *pc.lp;
    pgl_solve_kernel<<<1, PGL_TS, 0, stream>>>(pc.L, (int)lp.sp, w.sa, off, lp.C, lp.span, lp.F, lp.d, rec);
    pg_scan_launch12<false>(n, 1, PgLoadLoopDiff{N, E, pc.L, ptr, lst, lp.C, lp.span, lp.d}, w.sa, 6, w.bsum, rec, stream);
    pg_scan_apply_kernel<false><<<nb, PG_B, 0, stream>>>(n, w.sa, 6, off, PgFinDiffG{chain, lp.s, w.sb}, rec);
    pg_scan_launch12<false>(n, 1, PgLoadRow{w.sb}, w.sa, 6, w.bsum, rec, stream);
  }
  pg_scan_apply_kernel<false><<<nb, PG_B, 0, stream>>>(n, w.sa, 6, off, PgFinN{chain, out, r_for_dot, part}, rec);
  OVN_HIP_CHECK(hipGetLastError());
  return OVN_OK;
}

// `iterations` PCG iterations from iteration `first_iteration` (0: from the start) with the preconditioner `pc`
int pg_pcg(const PgPrecond& pc, const uint8_t* fixed, int N, const int32_t* ij, int E, const int32_t* ptr, const int32_t* lst,
           const double* blocks, const double* grad, const double* diag, double lambda, double rtol, int first_iteration, int iterations,
           double* delta, const PgWs& w, double* rec, hipStream_t s) {
  const int nbn = (N + PG_B - 1) / PG_B, nbc = (N - 1 + PG_B - 1) / PG_B;
  const int nbz = pc.chain ? nbc : nbn;   // the partials of r . z: per block of chain edges after the scans, else per block of nodes
  double* part = w.part_n;
  if (first_iteration == 0) {
    pg_solve_reset_kernel<<<1, 64, 0, s>>>(rec, pc.lp != nullptr);
    pg_solve_init_kernel<<<nbn, PG_B, 0, s>>>(fixed, N, grad, pc.dj, pc.scale, delta, w.r, w.z, w.p[0], w.p[1], part, rec);
    if (pc.chain) {
      int rc = pg_precond_apply(N, E, ptr, lst, pc, w.r, w.z, w, w.r, part, rec, s);
      if (rc) return rc;
    }
    pg_solve_rz0_kernel<<<1, PG_B, 0, s>>>(part, nbz, rec);
  }
  for (int k = 0; k < iterations; ++k) {
    const int cur = (first_iteration + k) & 1;
    pg_matvec_kernel<<<nbn, PG_B, 0, s>>>(fixed, N, ij, E, ptr, lst, blocks, diag, lambda, w.z, w.p[cur], w.p[cur ^ 1], w.q, part, rec);
    pg_alpha_kernel<<<1, PG_B, 0, s>>>(part, nbn, rec);
    pg_update_kernel<<<nbn, PG_B, 0, s>>>(N, w.p[cur ^ 1], w.q, pc.dj, pc.scale, delta, w.r, w.z, part, rec);
    if (pc.chain) {
      int rc = pg_precond_apply(N, E, ptr, lst, pc, w.r, w.z, w, w.r, part, rec, s);
      if (rc) return rc;
    }
    pg_beta_kernel<<<1, PG_B, 0, s>>>(part, nbz, rtol, rec);
  }
  OVN_HIP_CHECK(hipGetLastError());
  return OVN_OK;
}

// the argument checks the entries share; `fn` names the caller in the messages
int pg_check_lambda(const char* fn, double lambda) {
  OVN_REQUIRE(pg_finite(lambda) && lambda >= 0.0, OVN_ERR_ARG, "%s: lambda must be finite and >= 0", fn);
  return OVN_OK;
}
int pg_check_iterations(const char* fn, double lambda, double rtol, int first_iteration, int iterations) {
  if (int rc = pg_check_lambda(fn, lambda)) return rc;
  OVN_REQUIRE(pg_finite(rtol) && rtol >= 0.0, OVN_ERR_ARG, "%s: rtol must be finite and >= 0", fn);
  OVN_REQUIRE(first_iteration >= 0 && iterations >= 0 && iterations <= OVN_POSE_GRAPH_MAX_CHUNK, OVN_ERR_ARG,
              "%s: first_iteration %d (>= 0), iterations %d (0..%d)", fn, first_iteration, iterations, OVN_POSE_GRAPH_MAX_CHUNK);
  return OVN_OK;
}
// a chain of n_nodes - 1 edges and then the loop edges, at least `min_loops` of them
int pg_check_shape(const char* fn, int n_nodes, int n_edges, int n_loops, int min_loops) {
  OVN_REQUIRE(n_nodes >= 2 && n_nodes <= OVN_POSE_GRAPH_MAX_NODES && n_loops >= min_loops && n_loops <= OVN_POSE_GRAPH_MAX_LOOPS &&
                  (int64_t)n_edges == (int64_t)n_nodes - 1 + n_loops, OVN_ERR_ARG,
              "%s: %d nodes (2..%d), %d loop edges (%d..%d), %d edges (must be nodes - 1 + loop edges)", fn, n_nodes,
              OVN_POSE_GRAPH_MAX_NODES, n_loops, min_loops, OVN_POSE_GRAPH_MAX_LOOPS, n_edges);
  return OVN_OK;
}

// ---- marginal covariances (ovn_pose_graph_marginals; tests/_pose_graph_marginals_ref.py) -----------------------------
// Sigma_world(k) = Gamma[k] - Y_k' Y_k with L_S Y_k = V_k' and V_k = [(Gamma[clamp(k, lo_a, hi_a)] - Gamma[lo_a]) sigma_a C_a']_a: the
// diagonal blocks of H^-1 = H_c^-1 - H_c^-1 J' S^-1 J H_c^-1 in world tangent coordinates.  A workgroup owns PGM_TN queried nodes, 48
// columns, and walks the factor's block rows left-looking: X = V' block - sum_t F[kb][t] Y[t] (one subtraction of a 48-term sum in
// index order per earlier block, in block order), then the diagonal block column by column, one subtraction per column in column
// order.  Its Y tile lives in the workspace; the 48 x 48 blocks go through LDS.
// The diagonal-block solve shares no code with pgl_solve_kernel's: there one wave holds one vector in registers and shuffles, here
// four row groups work on 48 columns through LDS, and one form would change who computes what.
constexpr int PGM_TN = 8;                 // queried nodes per workgroup: 6 * 8 = PGL_NB columns
constexpr int PGM_CHUNK = 512;            // workgroups per launch: the Y tiles of one launch are what the workspace holds
constexpr int PGM_TRI = 21;               // entries of a 6 x 6 lower triangle
static_assert(6 * PGM_TN == PGL_NB, "a tile of queried nodes is one factor block wide");

struct PgMarg {   // the caller's ws_dev of ovn_pose_graph_marginals, in doubles
  double *gamma, *gsum, *Y, *part;
  int64_t nbc, nbq, tiles, chunk, sp;
  size_t total;
  PgMarg(double* base, int64_t N, int64_t L, int64_t K) {
    nbc = (N - 1 + PG_B - 1) / PG_B;
    nbq = (K + PG_B - 1) / PG_B;
    tiles = (K + PGM_TN - 1) / PGM_TN;
    chunk = tiles < PGM_CHUNK ? tiles : PGM_CHUNK;
    sp = (6 * L + PGL_NB - 1) / PGL_NB * PGL_NB;
    PgTake take{base};
    part = take(nbq);                              // out-of-range ids per finishing workgroup
    gamma = take(L == 0 ? 36 * N : 0);             // without loop edges nobody has scanned Gamma: a copy of its own
    gsum = take(L == 0 ? 72 * nbc : 0);
    Y = take((size_t)chunk * sp * PGL_NB);         // one (sp, 48) tile per workgroup of a launch
    total = take.o;
  }
};

// `breakdown` from the linearization's and the prepare's failed pivots, before anything touches cov; slot [15] starts at 0
__global__ void pgm_reset_kernel(double* rec, int L) {
  if (threadIdx.x != 0) return;
  rec[R_BREAK] = (rec[R_CHOL] != 0.0 || (L > 0 && rec[R_LPIV] != 0.0)) ? 1.0 : 0.0;
  rec[R_MOUT] = 0.0;
}

// the forward sweep of one launch: workgroup w owns queries q0 + 8 w .. q0 + 8 w + 7 and leaves the lower triangles of Y_k' Y_k in cov
__global__ __launch_bounds__(PG_B) void pgm_sweep_kernel(int N, int L, int sp, int64_t q0, int64_t K, const int32_t* __restrict__ ids,
                                                         const double* __restrict__ gamma, const double* __restrict__ C,
                                                         const double* __restrict__ span, const double* __restrict__ F,
                                                         double* __restrict__ Yws, double* __restrict__ cov, const double* rec) {
  if (rec[R_BREAK] != 0.0) return;
  __shared__ double A[PGL_NB][PGL_NB + 1], B[PGL_NB][PGL_NB + 1], Yd[PGL_NB][PGL_NB + 1];
  __shared__ int node[PGM_TN];
  __shared__ int fbs[PG_B];
  const int tid = threadIdx.x, nbk = sp / PGL_NB;
  const int64_t qb = q0 + (int64_t)blockIdx.x * PGM_TN;
  if (tid < PGM_TN) {
    int k = -1;
    if (qb + tid < K) {
      k = ids[qb + tid];
      if (k < 0 || k >= N) k = -1;
    }
    node[tid] = k;
  }
  __syncthreads();
  int kmax = -1;
#pragma unroll
  for (int n = 0; n < PGM_TN; ++n) kmax = max(kmax, node[n]);
  // the first block row in which some edge's V block is not zero for this tile: V_k's block a is zero for k <= lo_a
  int fb = nbk;
  for (int a = tid; a < L; a += PG_B)
    if (span[4 * a + 3] != 0.0 && (int)span[4 * a] < kmax) fb = min(fb, 6 * a / PGL_NB);
  fbs[tid] = fb;
  __syncthreads();
  for (int h = PG_B / 2; h > 0; h >>= 1) {
    if (tid < h) fbs[tid] = min(fbs[tid], fbs[tid + h]);
    __syncthreads();
  }
  fb = fbs[0];
  double* Yt = Yws + (size_t)blockIdx.x * sp * PGL_NB;
  const int tr = tid / 16 * 3, tc = tid % 16 * 3;     // this thread's 3 x 3 entries of a 48 x 48 block: rows tr.., columns tc..
  const int my = node[tc / 6], i0 = tc % 6;           // its three columns are rows i0 .. i0 + 2 of one node's V
  const int sc = tid % PGL_NB, sg = tid / PGL_NB;     // diagonal solve: column sc, rows sg, sg + 4, ... (threads 0 .. 191)
  int an = -1, ai = 0, aj = 0;                        // Y'Y: entry (ai, aj), ai >= aj, of node an (threads 0 .. 167)
  if (tid < PGM_TN * PGM_TRI) {
    an = tid / PGM_TRI;
    const int p = tid % PGM_TRI;
    while ((ai + 1) * (ai + 2) / 2 <= p) ++ai;
    aj = p - ai * (ai + 1) / 2;
  }
  double acc = 0.0;
  for (int kb = fb; kb < nbk; ++kb) {
    double x[3][3];
#pragma unroll
    for (int u = 0; u < 3; ++u)
#pragma unroll
      for (int v = 0; v < 3; ++v) x[u][v] = 0.0;
    const int r0 = kb * PGL_NB + tr, a = r0 / 6, qr = r0 % 6;   // its three rows are rows qr .. qr + 2 of edge a's C
    if (a < L && my >= 0 && span[4 * a + 3] != 0.0) {
      const int lo = (int)span[4 * a], hi = (int)span[4 * a + 1];
      if (my > lo) {
        const double* gh = gamma + (size_t)min(my, hi) * 36 + i0 * 6;
        const double* gl = gamma + (size_t)lo * 36 + i0 * 6;
        const double* cr = C + (size_t)a * 36 + qr * 6;
        const double sgn = span[4 * a + 2];
        double M[3][6];
#pragma unroll
        for (int v = 0; v < 3; ++v)
#pragma unroll
          for (int t = 0; t < 6; ++t) M[v][t] = gh[v * 6 + t] - gl[v * 6 + t];
#pragma unroll
        for (int u = 0; u < 3; ++u)
#pragma unroll
          for (int v = 0; v < 3; ++v) {
            double s = M[v][0] * cr[u * 6];
#pragma unroll
            for (int t = 1; t < 6; ++t) s = s + M[v][t] * cr[u * 6 + t];
            x[u][v] = sgn * s;
          }
      }
    }
    for (int t = fb; t < kb; ++t) {
      __syncthreads();
      pgl_stage_tile<PG_B, true>(A, F + (size_t)kb * PGL_NB * sp + (size_t)t * PGL_NB, sp,
                                 B, Yt + (size_t)t * PGL_NB * PGL_NB, PGL_NB);
      __syncthreads();
      double s[3][3];
      pgl_tile_mul3<false>(A, B, tr, tc, s);
#pragma unroll
      for (int u = 0; u < 3; ++u)
#pragma unroll
        for (int v = 0; v < 3; ++v) x[u][v] = x[u][v] - s[u][v];
    }
    __syncthreads();
    pgl_stage_tile<PG_B>(A, F + (size_t)kb * PGL_NB * sp + (size_t)kb * PGL_NB, sp);
#pragma unroll
    for (int u = 0; u < 3; ++u)
#pragma unroll
      for (int v = 0; v < 3; ++v) B[tr + u][tc + v] = x[u][v];
    __syncthreads();
    // the diagonal block: y_c = x_c / L_cc, then one subtraction per row below, column by column
    for (int c = 0; c < PGL_NB; ++c) {
      if (sg < 4) {
        const double y = B[c][sc] / A[c][c];
        if (c % 4 == sg) Yd[c][sc] = y;
        for (int r = c + 1 + ((sg - c - 1) % 4 + 4) % 4; r < PGL_NB; r += 4) B[r][sc] = B[r][sc] - A[r][c] * y;
      }
      __syncthreads();
    }
    for (int idx = tid; idx < PGL_NB * PGL_NB; idx += PG_B) {
      const int r = idx / PGL_NB, c = idx % PGL_NB;
      Yt[((size_t)kb * PGL_NB + r) * PGL_NB + c] = Yd[r][c];
    }
    if (an >= 0) {
#pragma unroll 4
      for (int r = 0; r < PGL_NB; ++r) acc = acc + Yd[r][6 * an + ai] * Yd[r][6 * an + aj];
    }
  }
  if (an >= 0 && qb + an < K) cov[(size_t)(qb + an) * 36 + ai * 6 + aj] = acc;
}

// one query per thread: Sigma_world = Gamma[k] - Y'Y on the lower triangle, mirrored; then A Sigma A' with A = Ad(T_k^-1) (local frame)
// or [[I, -p^], [0, I]] (position frame), its lower triangle mirrored.  Node 0 is all zeros; an id outside [0, N) gives NaNs and is counted
__global__ __launch_bounds__(PG_B) void pgm_finish_kernel(int N, int64_t K, int has_acc, int frame, const int32_t* __restrict__ ids,
                                                          const double* __restrict__ poses, const double* __restrict__ chain,
                                                          const double* __restrict__ gamma, double* __restrict__ cov,
                                                          double* __restrict__ part, const double* rec) {
  if (rec[R_BREAK] != 0.0) return;
  __shared__ double sh[PG_B];
  const int64_t q = (int64_t)blockIdx.x * PG_B + threadIdx.x;
  double bad = 0.0;
  if (q < K) {
    const int k = ids[q];
    double* out = cov + (size_t)q * 36;
    if (k < 0 || k >= N) {
      bad = 1.0;
      const double nan = __longlong_as_double(0x7ff8000000000000LL);
#pragma unroll
      for (int e = 0; e < 36; ++e) out[e] = nan;
    } else if (k == 0) {
#pragma unroll
      for (int e = 0; e < 36; ++e) out[e] = 0.0;
    } else {
      double Sg[36], Am[36], T[36];
      const double* g = gamma + (size_t)k * 36;
#pragma unroll
      for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) {
          const double v = has_acc ? g[i * 6 + j] - out[i * 6 + j] : g[i * 6 + j];
          Sg[i * 6 + j] = v;
          Sg[j * 6 + i] = v;
        }
      if (frame == OVN_POSE_GRAPH_COV_LOCAL) {
        ld36(chain + (size_t)(k - 1) * 72 + 36, Am);
      } else {
        const double* Tk = poses + (size_t)k * 16;
        const double p[3] = {Tk[3], Tk[7], Tk[11]};
        double H[9];
        m3_hat(p, H);
#pragma unroll
        for (int e = 0; e < 36; ++e) Am[e] = (e % 7 == 0) ? 1.0 : 0.0;
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
          for (int j = 0; j < 3; ++j) Am[i * 6 + 3 + j] = -H[i * 3 + j];
      }
      m6_mul(Am, Sg, T);
      m6_mult(T, Am, Sg);
#pragma unroll
      for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) {
          out[i * 6 + j] = Sg[i * 6 + j];
          out[j * 6 + i] = Sg[i * 6 + j];
        }
    }
  }
  const double b = pg_wg_sum(bad, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = b;
}
// ONE workgroup: record [15], the ids outside [0, N)
__global__ __launch_bounds__(PG_B) void pgm_record_kernel(const double* part, int nb, double* rec) {
  if (rec[R_BREAK] != 0.0) return;
  __shared__ double sh[PG_B];
  const double b = pg_partial_sum(part, nb, 1, sh);
  if (threadIdx.x == 0) rec[R_MOUT] = b;
}

}  // namespace

// ---- C ABI --------------------------------------------------------------------------------------------------------------------------------
extern "C" {

int64_t ovn_pose_graph_workspace_bytes(int64_t n_nodes, int64_t n_edges) {
  if (n_nodes < 1 || n_edges < 0 || n_nodes > OVN_POSE_GRAPH_MAX_NODES || n_edges > OVN_POSE_GRAPH_MAX_EDGES) return 0;
  return (int64_t)(PgWs(nullptr, n_nodes, n_edges).total * sizeof(double));
}

int ovn_pose_graph_linearize(ovn_ctx* ctx, void* stream, const double* poses_dev, const uint8_t* fixed_dev, int n_nodes,
                             const int32_t* edge_ij_dev, const double* meas_dev, const double* info_dev, int n_edges,
                             const int32_t* node_ptr_dev, const int32_t* node_edge_dev, double huber, double* res_dev, double* chi_dev,
                             double* weight_dev, double* jac_dev, double* blocks_dev, double* grad_dev, double* diag_dev,
                             double* dinv_dev, double* chain_dev, double* ws_dev, double* record_dev) {
  OVN_REQUIRE(ctx != nullptr, OVN_ERR_ARG, "ovn_pose_graph_linearize: ctx is NULL");
  OVN_REQUIRE(n_nodes >= 1 && n_nodes <= OVN_POSE_GRAPH_MAX_NODES && n_edges >= 0 && n_edges <= OVN_POSE_GRAPH_MAX_EDGES, OVN_ERR_ARG,
              "ovn_pose_graph_linearize: %d nodes (1..%d), %d edges (0..%d)", n_nodes, OVN_POSE_GRAPH_MAX_NODES, n_edges,
              OVN_POSE_GRAPH_MAX_EDGES);
  OVN_REQUIRE(huber > 0.0 && huber == huber, OVN_ERR_ARG, "ovn_pose_graph_linearize: huber must be > 0 (+inf: least squares)");
  OVN_REQUIRE(record_dev != nullptr, OVN_ERR_ARG, "ovn_pose_graph_linearize: record_dev is NULL");
  OVN_ON_DEVICE(ctx->device);
  hipStream_t s = (hipStream_t)stream;
  if (n_edges == 0) {   // nothing to measure: cost 0, no buffer but the record touched
    pg_set_record_kernel<<<1, 64, 0, s>>>(record_dev, R_COST, 4, 0.0);
    OVN_HIP_CHECK(hipGetLastError());
    return OVN_OK;
  }
  const bool jac = jac_dev != nullptr;
  OVN_REQUIRE(jac ? (blocks_dev && grad_dev && diag_dev && dinv_dev) : (!blocks_dev && !grad_dev && !diag_dev && !dinv_dev && !chain_dev),
              OVN_ERR_ARG, "ovn_pose_graph_linearize: jac, blocks, grad, diag and dinv are given together, or none of them (cost only)");
  OVN_REQUIRE(poses_dev && fixed_dev && edge_ij_dev && meas_dev && info_dev && res_dev && chi_dev && weight_dev && ws_dev, OVN_ERR_ARG,
              "ovn_pose_graph_linearize: NULL buffer");
  OVN_REQUIRE(!jac || (node_ptr_dev && node_edge_dev), OVN_ERR_ARG, "ovn_pose_graph_linearize: NULL incidence list");
  OVN_REQUIRE(!chain_dev || n_edges >= n_nodes - 1, OVN_ERR_ARG, "ovn_pose_graph_linearize: a chain needs the %d odometry edges first",
              n_nodes - 1);
  PgWs w(ws_dev, n_nodes, n_edges);
  const int nbe = (n_edges + PG_B - 1) / PG_B, nbn = (n_nodes + PG_B - 1) / PG_B;
  const int nbc = (chain_dev && n_nodes > 1) ? (n_nodes - 1 + PG_B - 1) / PG_B : 0;
  if (jac) {
    pg_edge_kernel<true><<<nbe, PG_B, 0, s>>>(poses_dev, n_nodes, edge_ij_dev, meas_dev, info_dev, n_edges, huber, res_dev, chi_dev,
                                              weight_dev, jac_dev, blocks_dev, w.eg, w.part_e);
    pg_node_kernel<<<nbn, PG_B, 0, s>>>(fixed_dev, n_nodes, edge_ij_dev, n_edges, node_ptr_dev, node_edge_dev, blocks_dev, w.eg, grad_dev,
                                        diag_dev, dinv_dev, w.part_n);
    if (nbc) pg_chain_kernel<<<nbc, PG_B, 0, s>>>(poses_dev, n_nodes, info_dev, weight_dev, jac_dev, chain_dev, w.part_c);
    pg_lin_record_kernel<<<1, PG_B, 0, s>>>(w.part_e, nbe, w.part_n, nbn, nbc ? w.part_c : nullptr, nbc, record_dev);
  } else {
    pg_edge_kernel<false><<<nbe, PG_B, 0, s>>>(poses_dev, n_nodes, edge_ij_dev, meas_dev, info_dev, n_edges, huber, res_dev, chi_dev,
                                               weight_dev, nullptr, nullptr, nullptr, w.part_e);
    pg_lin_record_kernel<<<1, PG_B, 0, s>>>(w.part_e, nbe, nullptr, 0, nullptr, 0, record_dev);
  }
  OVN_HIP_CHECK(hipGetLastError());
  return OVN_OK;
}

int ovn_pose_graph_solve(ovn_ctx* ctx, void* stream, const uint8_t* fixed_dev, int n_nodes, const int32_t* edge_ij_dev, int n_edges,
                         const int32_t* node_ptr_dev, const int32_t* node_edge_dev, const double* blocks_dev, const double* grad_dev,
                         const double* diag_dev, const double* dinv_dev, const double* chain_dev, int preconditioner, double lambda,
                         double rtol, int first_iteration, int iterations, double* delta_dev, double* ws_dev, double* record_dev) {
  OVN_REQUIRE(ctx != nullptr, OVN_ERR_ARG, "ovn_pose_graph_solve: ctx is NULL");
  OVN_REQUIRE(n_nodes >= 1 && n_nodes <= OVN_POSE_GRAPH_MAX_NODES && n_edges >= 0 && n_edges <= OVN_POSE_GRAPH_MAX_EDGES, OVN_ERR_ARG,
              "ovn_pose_graph_solve: %d nodes (1..%d), %d edges (0..%d)", n_nodes, OVN_POSE_GRAPH_MAX_NODES, n_edges,
              OVN_POSE_GRAPH_MAX_EDGES);
  OVN_REQUIRE(preconditioner == OVN_POSE_GRAPH_JACOBI || preconditioner == OVN_POSE_GRAPH_CHAIN, OVN_ERR_ARG,
              "ovn_pose_graph_solve: preconditioner %d (0 = block-Jacobi, 1 = odometry chain)", preconditioner);
  if (int rc = pg_check_iterations("ovn_pose_graph_solve", lambda, rtol, first_iteration, iterations)) return rc;
  OVN_REQUIRE(record_dev != nullptr, OVN_ERR_ARG, "ovn_pose_graph_solve: record_dev is NULL");
  OVN_ON_DEVICE(ctx->device);
  hipStream_t s = (hipStream_t)stream;
  if (n_edges == 0) {   // nothing to solve: converged after 0 iterations, delta untouched
    pg_set_record_kernel<<<1, 64, 0, s>>>(record_dev, R_ITER, 8, 0.0);
    pg_set_record_kernel<<<1, 64, 0, s>>>(record_dev, R_CONV, 1, 1.0);
    OVN_HIP_CHECK(hipGetLastError());
    return OVN_OK;
  }
  OVN_REQUIRE(fixed_dev && edge_ij_dev && node_ptr_dev && node_edge_dev && blocks_dev && grad_dev && diag_dev && dinv_dev && delta_dev &&
                  ws_dev, OVN_ERR_ARG, "ovn_pose_graph_solve: NULL buffer");
  const bool chain = preconditioner == OVN_POSE_GRAPH_CHAIN;
  OVN_REQUIRE(!chain || chain_dev, OVN_ERR_ARG, "ovn_pose_graph_solve: the chain preconditioner needs chain_dev");
  const PgPrecond pc = {chain ? nullptr : dinv_dev, 1.0 / (1.0 + lambda), chain ? chain_dev : nullptr, nullptr, 0};
  return pg_pcg(pc, fixed_dev, n_nodes, edge_ij_dev, n_edges, node_ptr_dev, node_edge_dev, blocks_dev, grad_dev, diag_dev, lambda, rtol,
                first_iteration, iterations, delta_dev, PgWs(ws_dev, n_nodes, n_edges), record_dev, s);
}

int ovn_pose_graph_precondition(ovn_ctx* ctx, void* stream, int n_nodes, int preconditioner, double lambda, const double* dinv_dev,
                                const double* chain_dev, const double* in_dev, double* out_dev, double* ws_dev) {
  OVN_REQUIRE(ctx != nullptr, OVN_ERR_ARG, "ovn_pose_graph_precondition: ctx is NULL");
  OVN_REQUIRE(n_nodes >= 1 && n_nodes <= OVN_POSE_GRAPH_MAX_NODES, OVN_ERR_ARG, "ovn_pose_graph_precondition: %d nodes (1..%d)", n_nodes,
              OVN_POSE_GRAPH_MAX_NODES);
  OVN_REQUIRE(preconditioner == OVN_POSE_GRAPH_JACOBI || preconditioner == OVN_POSE_GRAPH_CHAIN, OVN_ERR_ARG,
              "ovn_pose_graph_precondition: preconditioner %d (0 = block-Jacobi, 1 = odometry chain)", preconditioner);
  if (int rc = pg_check_lambda("ovn_pose_graph_precondition", lambda)) return rc;
  const bool chain = preconditioner == OVN_POSE_GRAPH_CHAIN;
  OVN_REQUIRE(in_dev && out_dev && ws_dev && (chain ? chain_dev != nullptr : dinv_dev != nullptr), OVN_ERR_ARG,
              "ovn_pose_graph_precondition: NULL buffer");
  OVN_ON_DEVICE(ctx->device);
  hipStream_t s = (hipStream_t)stream;
  if (!chain) {
    pg_jacobi_apply_kernel<<<(n_nodes + PG_B - 1) / PG_B, PG_B, 0, s>>>(n_nodes, dinv_dev, 1.0 / (1.0 + lambda), in_dev, out_dev);
    OVN_HIP_CHECK(hipGetLastError());
    return OVN_OK;
  }
  OVN_HIP_CHECK(hipMemsetAsync(out_dev, 0, 6 * sizeof(double), s));   // the fixed node 0
  const PgPrecond pc = {nullptr, 1.0, chain_dev, nullptr, 0};
  return pg_precond_apply(n_nodes, 0, nullptr, nullptr, pc, in_dev, out_dev, PgWs(ws_dev, n_nodes, 0), nullptr, nullptr, nullptr, s);
}

int ovn_pose_graph_retract(ovn_ctx* ctx, void* stream, const double* poses_dev, const uint8_t* fixed_dev, const double* delta_dev,
                           int n_nodes, double* out_dev, double* ws_dev, double* record_dev) {
  OVN_REQUIRE(ctx != nullptr, OVN_ERR_ARG, "ovn_pose_graph_retract: ctx is NULL");
  OVN_REQUIRE(n_nodes >= 1 && n_nodes <= OVN_POSE_GRAPH_MAX_NODES, OVN_ERR_ARG, "ovn_pose_graph_retract: %d nodes (1..%d)", n_nodes,
              OVN_POSE_GRAPH_MAX_NODES);
  OVN_REQUIRE(poses_dev && fixed_dev && delta_dev && out_dev && ws_dev && record_dev, OVN_ERR_ARG, "ovn_pose_graph_retract: NULL buffer");
  OVN_ON_DEVICE(ctx->device);
  hipStream_t s = (hipStream_t)stream;
  PgWs w(ws_dev, n_nodes, 0);
  const int nbn = (n_nodes + PG_B - 1) / PG_B;
  pg_retract_kernel<<<nbn, PG_B, 0, s>>>(poses_dev, fixed_dev, delta_dev, n_nodes, out_dev, w.part_n);
  pg_dmax_kernel<<<1, PG_B, 0, s>>>(w.part_n, nbn, record_dev);
  OVN_HIP_CHECK(hipGetLastError());
  return OVN_OK;
}

// ---- the chain-plus-loops inverse -------------------------------------------------------------------------------------------------------
int64_t ovn_pose_graph_loops_bytes(int64_t n_nodes, int64_t n_loops) {
  if (n_nodes < 2 || n_nodes > OVN_POSE_GRAPH_MAX_NODES || n_loops < 1 || n_loops > OVN_POSE_GRAPH_MAX_LOOPS) return 0;
  return (int64_t)(PgLoops(nullptr, n_nodes, n_loops).total * sizeof(double));
}

int ovn_pose_graph_loops_layout(int64_t n_nodes, int64_t n_loops, int64_t* out) {
  OVN_REQUIRE(out != nullptr, OVN_ERR_ARG, "ovn_pose_graph_loops_layout: out is NULL");
  OVN_REQUIRE(ovn_pose_graph_loops_bytes(n_nodes, n_loops) > 0, OVN_ERR_ARG, "ovn_pose_graph_loops_layout: %lld nodes, %lld loop edges",
              (long long)n_nodes, (long long)n_loops);
  double* const base = reinterpret_cast<double*>(sizeof(double));   // never dereferenced: offsets only
  PgLoops lp(base, n_nodes, n_loops);
  out[0] = PGL_NB;
  out[1] = lp.sp;
  out[2] = lp.gamma - base;
  out[3] = lp.C - base;
  out[4] = lp.winv - base;
  out[5] = lp.span - base;
  out[6] = lp.S - base;
  out[7] = lp.F - base;
  return OVN_OK;
}

int ovn_pose_graph_loops_prepare(ovn_ctx* ctx, void* stream, const double* poses_dev, int n_nodes, const int32_t* edge_ij_dev,
                                 const double* info_dev, const double* weight_dev, const double* jac_dev, int n_edges, int n_loops,
                                 const double* chain_dev, int stages, double* loops_dev, double* record_dev) {
  OVN_REQUIRE(ctx != nullptr, OVN_ERR_ARG, "ovn_pose_graph_loops_prepare: ctx is NULL");
  if (int rc = pg_check_shape("ovn_pose_graph_loops_prepare", n_nodes, n_edges, n_loops, 1)) return rc;
  OVN_REQUIRE(stages >= 1 && stages <= OVN_POSE_GRAPH_LOOPS_ALL, OVN_ERR_ARG, "ovn_pose_graph_loops_prepare: stages %d (a sum of 1 = scan, "
              "2 = assembly, 4 = factorization)", stages);
  OVN_REQUIRE(poses_dev && edge_ij_dev && info_dev && weight_dev && jac_dev && chain_dev && loops_dev && record_dev, OVN_ERR_ARG,
              "ovn_pose_graph_loops_prepare: NULL buffer");
  OVN_ON_DEVICE(ctx->device);
  hipStream_t s = (hipStream_t)stream;
  PgLoops lp(loops_dev, n_nodes, n_loops);
  const int nbl = (int)lp.nbl, sp = (int)lp.sp, nbk = (int)lp.nbk, n6 = 6 * n_loops;
  if (stages & OVN_POSE_GRAPH_LOOPS_SCAN) pg_gamma_scan(n_nodes - 1, chain_dev, lp.gamma, lp.gsum, s);
  if (stages & OVN_POSE_GRAPH_LOOPS_ASSEMBLE) {
    pgl_edge_kernel<<<nbl, PG_B, 0, s>>>(poses_dev, n_nodes, edge_ij_dev, info_dev, weight_dev, jac_dev, n_loops, lp.C, lp.winv, lp.span,
                                         lp.part);
    pgl_assemble_kernel<<<dim3(nbl, n_loops), PG_B, 0, s>>>(n_loops, sp, lp.gamma, lp.C, lp.winv, lp.span, lp.S, lp.F);
    if (sp > n6) pgl_pad_kernel<<<(int)(((int64_t)(sp - n6) * sp + PG_B - 1) / PG_B), PG_B, 0, s>>>(n6, sp, lp.S, lp.F);
  }
  for (int k = 0; k < ((stages & OVN_POSE_GRAPH_LOOPS_FACTOR) ? nbk : 0); ++k) {
    pgl_panel_kernel<<<1, 64, 0, s>>>(sp, k, lp.F, lp.pf);
    const int rest = nbk - 1 - k;
    if (rest > 0) {
      pgl_trsm_kernel<<<(rest * PGL_NB + PG_B - 1) / PG_B, PG_B, 0, s>>>(sp, k, lp.F);
      pgl_syrk_kernel<<<dim3(rest, rest), PG_B, 0, s>>>(sp, k, lp.F);
    }
  }
  if (stages & OVN_POSE_GRAPH_LOOPS_FACTOR) pgl_record_kernel<<<1, 64, 0, s>>>(lp.part, nbl, lp.pf, nbk, record_dev);
  OVN_HIP_CHECK(hipGetLastError());
  return OVN_OK;
}

int ovn_pose_graph_solve_loops(ovn_ctx* ctx, void* stream, const uint8_t* fixed_dev, int n_nodes, const int32_t* edge_ij_dev, int n_edges,
                               const int32_t* node_ptr_dev, const int32_t* node_edge_dev, const double* blocks_dev, const double* grad_dev,
                               const double* diag_dev, const double* dinv_dev, const double* chain_dev, double* loops_dev, int n_loops,
                               double lambda, double rtol, int first_iteration, int iterations, double* delta_dev, double* ws_dev,
                               double* record_dev) {
  OVN_REQUIRE(ctx != nullptr, OVN_ERR_ARG, "ovn_pose_graph_solve_loops: ctx is NULL");
  if (int rc = pg_check_shape("ovn_pose_graph_solve_loops", n_nodes, n_edges, n_loops, 1)) return rc;
  if (int rc = pg_check_iterations("ovn_pose_graph_solve_loops", lambda, rtol, first_iteration, iterations)) return rc;
  OVN_REQUIRE(fixed_dev && edge_ij_dev && node_ptr_dev && node_edge_dev && blocks_dev && grad_dev && diag_dev && dinv_dev && chain_dev &&
                  loops_dev && delta_dev && ws_dev && record_dev, OVN_ERR_ARG, "ovn_pose_graph_solve_loops: NULL buffer");
  OVN_ON_DEVICE(ctx->device);
  hipStream_t s = (hipStream_t)stream;
  const PgLoops lp(loops_dev, n_nodes, n_loops);
  const PgPrecond pc = {nullptr, 1.0, chain_dev, &lp, n_loops};
  return pg_pcg(pc, fixed_dev, n_nodes, edge_ij_dev, n_edges, node_ptr_dev, node_edge_dev, blocks_dev, grad_dev, diag_dev, lambda, rtol,
                first_iteration, iterations, delta_dev, PgWs(ws_dev, n_nodes, n_edges), record_dev, s);
}

int ovn_pose_graph_precondition_loops(ovn_ctx* ctx, void* stream, int n_nodes, int n_edges, int n_loops, const int32_t* node_ptr_dev,
                                      const int32_t* node_edge_dev, const double* chain_dev, double* loops_dev, const double* in_dev,
                                      double* out_dev, double* ws_dev) {
  OVN_REQUIRE(ctx != nullptr, OVN_ERR_ARG, "ovn_pose_graph_precondition_loops: ctx is NULL");
  if (int rc = pg_check_shape("ovn_pose_graph_precondition_loops", n_nodes, n_edges, n_loops, 1)) return rc;
  OVN_REQUIRE(node_ptr_dev && node_edge_dev && chain_dev && loops_dev && in_dev && out_dev && ws_dev, OVN_ERR_ARG,
              "ovn_pose_graph_precondition_loops: NULL buffer");
  OVN_ON_DEVICE(ctx->device);
  hipStream_t s = (hipStream_t)stream;
  OVN_HIP_CHECK(hipMemsetAsync(out_dev, 0, 6 * sizeof(double), s));   // the fixed node 0
  const PgLoops lp(loops_dev, n_nodes, n_loops);
  const PgPrecond pc = {nullptr, 1.0, chain_dev, &lp, n_loops};
  return pg_precond_apply(n_nodes, n_edges, node_ptr_dev, node_edge_dev, pc, in_dev, out_dev, PgWs(ws_dev, n_nodes, 0), nullptr, nullptr,
                          nullptr, s);
}

// ---- marginal covariances ---------------------------------------------------------------------------------------------------------------
int64_t ovn_pose_graph_marginals_bytes(int64_t n_nodes, int64_t n_loops, int64_t n_query) {
  if (n_nodes < 2 || n_nodes > OVN_POSE_GRAPH_MAX_NODES || n_loops < 0 || n_loops > OVN_POSE_GRAPH_MAX_LOOPS || n_query < 1 ||
      n_query > OVN_POSE_GRAPH_MAX_QUERY)
    return 0;
  return (int64_t)(PgMarg(nullptr, n_nodes, n_loops, n_query).total * sizeof(double));
}

int ovn_pose_graph_marginals(ovn_ctx* ctx, void* stream, const double* poses_dev, int n_nodes, int n_edges, int n_loops,
                             const double* chain_dev, const double* loops_dev, const int32_t* node_ids_dev, int64_t n_query, int frame,
                             double* cov_dev, double* ws_dev, double* record_dev) {
  OVN_REQUIRE(ctx != nullptr, OVN_ERR_ARG, "ovn_pose_graph_marginals: ctx is NULL");
  if (int rc = pg_check_shape("ovn_pose_graph_marginals", n_nodes, n_edges, n_loops, 0)) return rc;
  OVN_REQUIRE(n_query >= 1 && n_query <= OVN_POSE_GRAPH_MAX_QUERY, OVN_ERR_ARG, "ovn_pose_graph_marginals: %lld queried nodes (1..%d)",
              (long long)n_query, OVN_POSE_GRAPH_MAX_QUERY);
  OVN_REQUIRE(frame == OVN_POSE_GRAPH_COV_LOCAL || frame == OVN_POSE_GRAPH_COV_POSITION, OVN_ERR_ARG,
              "ovn_pose_graph_marginals: frame %d (0 = local, 1 = position)", frame);
  OVN_REQUIRE(poses_dev && chain_dev && node_ids_dev && cov_dev && ws_dev && record_dev && (n_loops == 0 || loops_dev), OVN_ERR_ARG,
              "ovn_pose_graph_marginals: NULL buffer");
  OVN_ON_DEVICE(ctx->device);
  hipStream_t s = (hipStream_t)stream;
  PgMarg m(ws_dev, n_nodes, n_loops, n_query);
  pgm_reset_kernel<<<1, 64, 0, s>>>(record_dev, n_loops);
  const double* gamma = m.gamma;
  if (n_loops == 0) {   // dead reckoning: Gamma alone, scanned here
    pg_gamma_scan(n_nodes - 1, chain_dev, m.gamma, m.gsum, s);
  } else {
    PgLoops lp(const_cast<double*>(loops_dev), n_nodes, n_loops);
    gamma = lp.gamma;
    for (int64_t t0 = 0; t0 < m.tiles; t0 += PGM_CHUNK) {
      const int64_t nt = m.tiles - t0 < PGM_CHUNK ? m.tiles - t0 : PGM_CHUNK;
      pgm_sweep_kernel<<<(int)nt, PG_B, 0, s>>>(n_nodes, n_loops, (int)lp.sp, t0 * PGM_TN, n_query, node_ids_dev, lp.gamma, lp.C, lp.span,
                                                lp.F, m.Y, cov_dev, record_dev);
    }
  }
  pgm_finish_kernel<<<(int)m.nbq, PG_B, 0, s>>>(n_nodes, n_query, n_loops > 0, frame, node_ids_dev, poses_dev, chain_dev, gamma, cov_dev,
                                                m.part, record_dev);
  pgm_record_kernel<<<1, PG_B, 0, s>>>(m.part, (int)m.nbq, record_dev);
  OVN_HIP_CHECK(hipGetLastError());
  return OVN_OK;
}

}  // extern "C"
