// After the path beyond the eigensolver's size (uglad_conditional_mean_wide: every D up to the cell's own limit), fp64 throughout: the
// conditional Gaussian / MAP estimate given observed coordinates (main.py:1176-1260) as a second client of chol_wide.h's tile layer and
// blocked Cholesky.  after_path.h's map_solve_kernel inverts the masked matrix with the one-workgroup eigensolver and stops at D = 256;
// L_uu is symmetric positive definite in every legitimate call, so a Cholesky factorisation gives solve, inverse and log-determinant.
//
// Problem k works on the masked matrix of map_prepare_kernel: A_ij = P_ij where i and j are both unobserved, delta_ij otherwise, padded
// with the identity to DP = D rounded up to 64.  A^-1 carries L_uu^-1 on the (u, u) block and the identity elsewhere: no gather / scatter.
//
//   afterw_prepare_kernel   one workgroup per 64 x 64 tile: A from the UPPER triangle of P, mirrored (as the small path); and the tile's part
//                           of r_u = sum_{j observed} P_uj (x_j - mean_j), columns over waves combined in wave order
//   afterw_rhs_kernel       r = the parts summed over the block columns in order (0 on observed coordinates and in the padding); the control
//                           block of the factorisation (sigma = 0, active, not flagged)
//   cholw_update_kernel, cholw_panel_kernel<CholwInvView>
//                           A = L L^T, two launches per block column, which also leave L(j, j)^-T and the log-pivots (chol_wide.h).  A pivot
//                           that is <= 0 or NaN raises the problem's flag; every later gated launch returns at once for it
//   afterw_subst_kernel     W = L^-1 by block forward substitution, one launch per block row i: W(i, j) = -L(i, i)^-1 sum_{j <= p < i} L(i, p) W(p, j)
//                           for all j < i, a tile product and a 64 x 64 triangular multiply.  W is kept TRANSPOSED (Wt = L^-T, block upper
//                           triangular): then both operands of every tile product here and in afterw_cov_kernel run along k, like rows of L
//   afterw_matvec_kernel    y = W^T (W r) and one step of refinement y += W^T (W (r - A y)): five matrix-vector launches, a workgroup per 64
//                           outputs.  Down a column (W v, A v): lane = output, rows over waves combined in wave order; along a row (W^T v):
//                           a wave per output, the lanes' partial sums combined by the butterfly of wave_sum_f64
//   afterw_cov_kernel       (only when the caller wants cond_cov) X = W^T W on the upper tiles, k from the later block row on; rounded once to
//                           fp32 and both triangles stored from the same value; observed rows / columns are exactly the identity
//   afterw_finish_kernel    full_mean_i = value_i where observed, mean_i - y_i otherwise (clip01: clamped to [0, 1]);
//                           log_pdf = -n_u / 2 log 2 pi + 1/2 sum log pivot (observed and padded pivots are exactly 1)
//
// L_uu not positive definite (or NaN): log_pdf = NaN, the unobserved entries of full_mean and the (u, u) block of cond_cov are NaN, observed
// entries still pass through; nothing aborts and the other problems of the batch are unaffected.  (The reference's multivariate_normal.pdf
// raises there.)
// Deviations from a plain reading of the plan: W is stored transposed (above); the log-pivots are summed as 256 strided partial sums combined
// in thread order rather than one chain in index order -- still one fixed order.
// Every sum has a fixed order, so results are bit-reproducible and independent of the batch.  Nothing reads back to the host: the sequence
// (2 + 2 nt + (nt - 1) + 5 + 1 + 1 launches, nt = DP / 64) is one linear chain and can be captured into a graph.
#pragma once
#include "chol_wide.h"

namespace uglad {

// A problem's part of the workspace, in DOUBLES (the buffer is 8-byte aligned; DP = D rounded up to 64): the factorisation's slab with the
// inverse (CholwInvView) --
//   A     DP x DP   the masked precision matrix, identity on the observed coordinates and in the padding
//   L     DP x DP   its Cholesky factor: the tiles below the block diagonal
//   r | y | t   3 DP   right-hand side, solution, intermediate
//   CholwCtl   8   only the "not PD" flag is live (sigma = 0, always active)
//   Wt    DP x DP   L^-T, block upper triangular
//   log pivots   DP
// -- and behind it
//   residual   DP   the fourth vector
//   parts of r   DP / 64 x DP   one row per block column of A
struct AfterwView {
  CholwInvView c;
  enum Vec { kR = 0, kY = 1, kT = 2, kRes = 3 };
  __host__ __device__ double* vec(int t, int which) const { return which < 3 ? c.vec3(t) + (size_t)which * c.DP : c.log_pivot(t) + c.DP; }
  __host__ __device__ double* rparts(int t) const { return c.log_pivot(t) + 2 * (size_t)c.DP; }  // [DP / 64][DP]
};
__host__ __device__ constexpr size_t afterw_problem_doubles(int DP) {
  return cholw_slab_doubles(DP) + (size_t)DP * DP + 2 * (size_t)DP + (size_t)(DP / kT64) * DP;
}
// (the friend that chol_wide.h's CholwInvView names: the one place that view is made)
__host__ inline AfterwView afterw_view(float* workspace, int D) {
  const int DP = t64_padded(D);
  return AfterwView{CholwInvView(CholwView{reinterpret_cast<double*>(workspace), afterw_problem_doubles(DP), DP})};
}
__host__ inline size_t afterw_problem_floats(int D) { return 2 * afterw_problem_doubles(t64_padded(D)); }

struct AfterwIn {
  const double* P;       // (K, D, D), the upper triangle is read
  const double* mean;    // (K, D)
  const float* observed;  // (K, D): non-zero where observed
  const double* values;  // (K, D): read where observed
};

// ---------------------------------------------------------------------------------------------------------------- A and the parts of r
// grid (DP / 64, DP / 64, K): tile (I, J) = (blockIdx.y, blockIdx.x).  The tile (min, max) of P goes through LDS, so the lower tiles are
// the transposes of the upper ones to the bit.
__global__ __launch_bounds__(kWThreads) void afterw_prepare_kernel(AfterwIn in, int D, AfterwView v) {
  __shared__ double s_p[kT64 * kT64Ldt], s_d[kT64], s_part[4][kT64];
  __shared__ int s_ob[2][kT64];
  const int I = blockIdx.y, J = blockIdx.x, t = blockIdx.z, DP = v.c.DP;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const bool upper = I <= J;
  const int a0 = (upper ? I : J) * kT64, b0 = (upper ? J : I) * kT64;  // the tile of P that is read
  const double* Pt = in.P + (size_t)t * D * D;
  const float* ob = in.observed + (size_t)t * D;
  t64_for_each_element([&](int a, int b) { s_p[a * kT64Ldt + b] = (a0 + a < D && b0 + b < D) ? Pt[(size_t)(a0 + a) * D + b0 + b] : 0.0; });
  if (tid < kT64) {
    const int i = I * kT64 + tid, j = J * kT64 + tid;
    s_ob[0][tid] = i >= D || ob[i] != 0.f;  // (the padding counts as observed: identity, no part in r)
    const bool obj = j < D && ob[j] != 0.f;
    s_ob[1][tid] = j >= D || obj;
    s_d[tid] = obj ? in.values[(size_t)t * D + j] - in.mean[(size_t)t * D + j] : 0.0;
  }
  __syncthreads();
  // element (x, y) of the symmetric matrix's tile (I, J): from the upper triangle
  auto el = [&](int x, int y) {
    if (I == J) return x <= y ? s_p[x * kT64Ldt + y] : s_p[y * kT64Ldt + x];
    return upper ? s_p[x * kT64Ldt + y] : s_p[y * kT64Ldt + x];
  };
  double* A = v.c.a(t);
  t64_for_each_element([&](int x, int y) {
    const bool keep = !s_ob[0][x] && !s_ob[1][y];
    A[(size_t)(I * kT64 + x) * DP + J * kT64 + y] = keep ? el(x, y) : ((I == J && x == y) ? 1.0 : 0.0);
  });
  // r's part from this block column: row = lane, columns w, w + 4, ...; the four partial sums combined in wave order
  double part = 0.0;
  for (int y = w; y < kT64; y += 4)
    if (s_ob[1][y]) part = fma(el(lane, y), s_d[y], part);  // (s_d is 0 in the padding)
  part = t64_sum_waves(part, s_part);
  if (w == 0) v.rparts(t)[(size_t)J * DP + I * kT64 + lane] = part;
}

// grid (DP / 64, K), 64 threads
__global__ __launch_bounds__(64) void afterw_rhs_kernel(const float* __restrict__ observed, int D, AfterwView v) {
  const int t = blockIdx.y, i = blockIdx.x * kT64 + threadIdx.x, DP = v.c.DP;
  double r = 0.0;
  if (i < D && observed[(size_t)t * D + i] == 0.f) {
    const double* parts = v.rparts(t);
    for (int J = 0; J < DP / kT64; ++J) r += parts[(size_t)J * DP + i];
  }
  v.vec(t, AfterwView::kR)[i] = r;
  if (i == 0) v.c.ctl(t)->reset(0.0);
}

// ---------------------------------------------------------------------------------------------------------------- W = L^-1, block row i
// grid (i, K): tile (i, j), j = blockIdx.x < i.  T = sum_{64 j <= k < 64 i} L(i0 + x, k) Wt(j0 + y, k); Wt(j0 + y, i0 + x) = -sum_{q <= x}
// M(x, q) T(q, y) with M = L(i, i)^-1, read from its transpose in tile (i, i) of Wt (written by the panel launch of block column i).
// This launch writes block column i of Wt and reads block columns j .. i - 1 of it.
__global__ __launch_bounds__(kWThreads) void afterw_subst_kernel(int i, AfterwView v) {
  __shared__ __attribute__((aligned(16))) double s_stage[2 * kT64Stage];
  __shared__ double s_m[kT64 * kT64Ldt];
  const int t = blockIdx.y;
  if (!cholw_gate(v.c.ctl(t))) return;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, DP = v.c.DP;
  const int j = blockIdx.x, i0 = i * kT64, j0 = j * kT64;
  const double* L = v.c.l(t);
  double* Wt = v.c.inv_t(t);
  const double* rows[2] = {L + (size_t)i0 * DP, Wt + (size_t)j0 * DP};
  f64x4 acc[2][2];
  t64_zero(acc);
  t64_tile_product<true>(j0, i0, [&](int which, int x, int k) { return rows[which][(size_t)x * DP + k]; }, s_stage, s_stage + kT64Stage, acc);
  t64_for_each_element([&](int q, int x) { s_m[x * kT64Ldt + q] = Wt[(size_t)(i0 + q) * DP + i0 + x]; });  // s_m[x][q] = M(x, q) = Wt(i0 + q, i0 + x)
  __syncthreads();  // (the last chunk has been consumed: the staging area becomes T, [q][y] with row stride kT64Ldt)
  double* s_tt = s_stage;
  static_assert(kT64 * kT64Ldt <= 2 * kT64Stage, "T fits the staging area");
  t64_for_each_fragment([&](int a, int c, int r, int row, int col) { s_tt[row * kT64Ldt + col] = acc[a][c][r]; });
  __syncthreads();
  // thread = row x (lane) x columns y = w, w + 4, ...: the stores run along x, a row of Wt
  for (int y = w; y < kT64; y += 4) {
    double s = 0.0;
    for (int q = 0; q <= lane; ++q) s = fma(s_m[lane * kT64Ldt + q], s_tt[q * kT64Ldt + y], s);
    Wt[(size_t)(j0 + y) * DP + i0 + lane] = -s;
  }
}

// ---------------------------------------------------------------------------------------------------------------- matrix-vector steps
// grid (DP / 64, K): outputs i0 .. i0 + 63 of  out = M v  over k0 <= k < k1.
//   kRows = false: out_i = sum_k Mx[k][i] v_k (down a column of the slab): lane = output, rows w, w + 4, ... per wave, combined in wave order
//   kRows = true : out_i = sum_k Mx[i][k] v_k (along a row): wave w takes outputs w, w + 4, ...; lanes stride k; wave_sum_f64
// which: 0  t = W v (Wt down the columns, k < i0 + 64)   1  y (+)= W^T t (Wt along the rows, k >= i0)   2  res = r - A y (A is symmetric)
enum { kAfterwLower = 0, kAfterwUpper = 1, kAfterwResidual = 2 };
template <bool kRows>
__global__ __launch_bounds__(kWThreads) void afterw_matvec_kernel(int which, int src, int dst, int accumulate, AfterwView v) {
  __shared__ double s_part[4][kT64];
  const int t = blockIdx.y;
  if (!cholw_gate(v.c.ctl(t))) return;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, DP = v.c.DP, i0 = blockIdx.x * kT64;
  const double* Mx = which == kAfterwResidual ? v.c.a(t) : v.c.inv_t(t);
  const double* x = v.vec(t, src);
  double* out = v.vec(t, dst);
  const int k0 = which == kAfterwUpper ? i0 : 0, k1 = which == kAfterwLower ? i0 + kT64 : DP;
  if constexpr (kRows) {
    for (int o = w; o < kT64; o += 4) {
      const double* row = Mx + (size_t)(i0 + o) * DP;
      double s = 0.0;
      for (int k = k0 + lane; k < k1; k += 64) s = fma(row[k], x[k], s);
      s = wave_sum_f64(s);
      if (lane == 0) out[i0 + o] = accumulate ? out[i0 + o] + s : s;
    }
  } else {
    const double* col = Mx + i0 + lane;
    double s = 0.0;
    int k = k0 + w;
    for (; k + 12 < k1; k += 16) {  // four loads in flight, one fma chain in k order
      const double m0 = col[(size_t)k * DP], m1 = col[(size_t)(k + 4) * DP], m2 = col[(size_t)(k + 8) * DP], m3 = col[(size_t)(k + 12) * DP];
      s = fma(m0, x[k], s);
      s = fma(m1, x[k + 4], s);
      s = fma(m2, x[k + 8], s);
      s = fma(m3, x[k + 12], s);
    }
    for (; k < k1; k += 4) s = fma(col[(size_t)k * DP], x[k], s);
    const double sum = t64_sum_waves(s, s_part);
    if (w == 0) {
      out[i0 + lane] = which == kAfterwResidual ? v.vec(t, AfterwView::kR)[i0 + lane] - sum : sum;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- cond_cov = A^-1
// grid (DP / 64, DP / 64, K); tiles below the diagonal return.  X(I, J) = sum_{k >= 64 J} Wt(I0 + x, k) Wt(J0 + y, k).  Not gated: a flagged
// problem gets NaN on its (u, u) block.
__global__ __launch_bounds__(kWThreads) void afterw_cov_kernel(const float* __restrict__ observed, int D, AfterwView v, float* __restrict__ cond_cov) {
  __shared__ __attribute__((aligned(16))) double s_stage[2 * kT64Stage];
  const int I = blockIdx.y, J = blockIdx.x, t = blockIdx.z;
  if (I > J) return;  // (uniform per workgroup)
  const bool ok = cholw_gate(v.c.ctl(t));
  const int DP = v.c.DP;
  const double* Wt = v.c.inv_t(t);
  const double* rows[2] = {Wt + (size_t)I * kT64 * DP, Wt + (size_t)J * kT64 * DP};
  f64x4 acc[2][2];
  t64_zero(acc);
  if (ok)
    t64_tile_product<true>(J * kT64, DP, [&](int which, int x, int k) { return rows[which][(size_t)x * DP + k]; }, s_stage, s_stage + kT64Stage, acc);
  const float* ob = observed + (size_t)t * D;
  float* C = cond_cov + (size_t)t * D * D;
  t64_for_each_fragment([&](int a, int c, int r, int row, int col) {
    const int i = I * kT64 + row, j = J * kT64 + col;
    if (i > j || j >= D) return;  // (the diagonal tile: its lower half is the mirror of its upper half)
    const float val = (ob[j] != 0.f || ob[i] != 0.f) ? (i == j ? 1.f : 0.f) : (ok ? (float)acc[a][c][r] : __builtin_nanf(""));
    C[(size_t)i * D + j] = val;
    if (i != j) C[(size_t)j * D + i] = val;
  });
}

// ---------------------------------------------------------------------------------------------------------------- full_mean and log_pdf
// grid (DP / 64, K), 256 threads.  Not gated.  Workgroup 0 of a problem also writes log_pdf (when asked for).
__global__ __launch_bounds__(kWThreads) void afterw_finish_kernel(AfterwIn in, int D, int clip01, AfterwView v, double* __restrict__ full_mean,
                                                                 double* __restrict__ log_pdf) {
  __shared__ double s_sum[kWThreads];
  __shared__ int s_nu[kWThreads];
  const int t = blockIdx.y, tid = threadIdx.x, DP = v.c.DP;
  const bool ok = cholw_gate(v.c.ctl(t));
  const float* ob = in.observed + (size_t)t * D;
  const int i = blockIdx.x * kT64 + tid;
  if (tid < kT64 && i < D) {
    double val;
    if (ob[i] != 0.f) val = in.values[(size_t)t * D + i];
    else val = ok ? in.mean[(size_t)t * D + i] - v.vec(t, AfterwView::kY)[i] : __builtin_nan("");
    if (clip01 && val == val) val = fmin(fmax(val, 0.0), 1.0);  // (NaN stays NaN)
    full_mean[(size_t)t * D + i] = val;
  }
  if (blockIdx.x != 0 || !log_pdf) return;  // (uniform per workgroup)
  int nu = 0;
  for (int k = tid; k < D; k += kWThreads) nu += ob[k] == 0.f;
  s_nu[tid] = nu;
  const double sum = cholw_log_pivot_sum(v.c, t, DP, ok, s_sum);  // (its barrier publishes s_nu; NaN for a flagged problem)
  if (tid == 0) {
    int n = 0;
    for (int k = 0; k < kWThreads; ++k) n += s_nu[k];
    log_pdf[t] = fma(-0.5 * (double)n, 1.8378770664093453, 0.5 * sum);
  }
}

}  // namespace uglad
