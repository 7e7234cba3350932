// Scoring rows against fitted models (uglad_sample_scores: every 1 <= D up to the cell's own limit), fp64 throughout: the squared
// Mahalanobis distance and the Gaussian log-density of each of N rows under each of K models (precision Theta, location mu) -- what
// sklearn's covariance estimators call mahalanobis(X) and score_samples(X).  A third client of chol_wide.h's tile layer and blocked Cholesky.
//
//   P = (Theta + Theta^T) / 2        formed in fp64 when the model is loaded (exact for fp32-born values; a converged precision_ is
//                                    asymmetric at 1e-5), xc = x - mu (one fp64 subtraction),
//   q = xc^T P xc,   log-density = (logdet P - D log 2 pi - q) / 2.
//
//   scorew_prepare_kernel   one workgroup per 64 x 64 tile: P into the factorisation's slab A (row stride DP = D rounded up to 64, identity
//                           in the padding) by chol_wide.h's t64_symmetric_part, so P is symmetric to the bit; the control block of the
//                           factorisation (sigma = 0, active, not flagged)
//   scorew_quad_kernel      grid (ceil(N / 64), DP / 64, K): one workgroup owns 64 rows of the table and one block column J of P.
//                           acc = sum_{I <= J} w Xc[rows, I] P[I, J] on the fp64 MFMA, k = 0 .. 64 (J + 1), w = 2 for I < J and 1 for I = J
//                           applied where the P operand is loaded (exact): the symmetry halves the flops.  P[j][.] is contiguous along k,
//                           so both operands take the [x][k] layout.  The fragments times Xc[row, 64 J + col] are summed per row -- a
//                           lane's two columns, the sixteen lanes of a row by a butterfly, the two waves of a row through LDS in wave
//                           order -- into ONE partial per (model, J, row).  Ragged N and D are zero-filled AFTER centring.  Block columns
//                           are dealt out from the last (heaviest) to the first.
//   cholw_update_kernel, cholw_panel_kernel<CholwInvView>
//                           (only when the caller wants log_density or logdet) P = L L^T on after_wide.h's layout, whose view carries the
//                           log-pivots (chol_wide.h).  A pivot that is <= 0 or NaN raises the model's flag
//   scorew_logdet_kernel    logdet P = the D log-pivots (cholw_log_pivot_sum, as afterw_finish_kernel); NaN for a flagged model
//   scorew_finish_kernel    q[n] = the partials summed over J = 0 .. DP / 64 - 1 in ascending order, then the log-density
//
// THE BITWISE PROPERTY.  A row's two numbers depend on that row and the model alone: not on N, not on the row's position in the table, not
// on K or the model's place in the batch, not on the grid.  Every element of the tile product is the same k-ordered fma chain whatever its
// place in the tile, every row of a tile is reduced by the same tree, and the partials -- T / D = 1 / 64 of the table's own bytes -- are
// combined in index order.  So a table may be scored in chunks of rows, in any order, and the bits do not change; a NaN in one row stays in
// that row.
// P not positive definite (or NaN): logdet and every log-density of that model are NaN, its q values are still returned, and the other
// models of the batch are unaffected.  Nothing reads back to the host: 2 + 2 + 2 DP / 64 launches in one chain.
#pragma once
#include "after_wide.h"

namespace uglad {

// The workspace, in DOUBLES (the buffer is 8-byte aligned): K problems of after_wide.h's layout (A = P, L, the control block, the log-pivots;
// vector 0 of vec3 carries logdet P in its first element), and behind them the partials, (K, DP / 64, NP) with NP = N rounded up to 64.
__host__ __device__ constexpr size_t scorew_padded_rows(int N) { return ((size_t)N + kT64 - 1) / kT64 * kT64; }
__host__ inline size_t scorew_model_floats(int N, int D) {  // (per model: its problem and its partials; the K problems lie in front of all partials)
  const int DP = t64_padded(D);
  return 2 * (afterw_problem_doubles(DP) + (size_t)(DP / kT64) * scorew_padded_rows(N));
}
__host__ inline double* scorew_partials(const AfterwView& v, int K) { return v.c.base + (size_t)K * v.c.stride; }

struct ScorewIn {
  const double* X;     // (x_batch, N, D)
  const double* mean;  // (K, D)
  int x_batch;         // K, or 1: one table for every model
  int N, D;
  __device__ const double* table(int t) const { return X + (x_batch == 1 ? (size_t)0 : (size_t)t * N * D); }
};

// ---------------------------------------------------------------------------------------------------------------- P and the control block
// grid (DP / 64, DP / 64, K): tile (I, J) = (blockIdx.y, blockIdx.x) of P, the identity in the padding
__global__ __launch_bounds__(kWThreads) void scorew_prepare_kernel(const double* __restrict__ theta, int D, AfterwView v) {
  const int I = blockIdx.y, J = blockIdx.x, t = blockIdx.z, DP = v.c.DP;
  double* A = v.c.a(t);
  t64_symmetric_part(theta + (size_t)t * D * D, D, I, J, [&](int x, int y, double val, bool inside) {
    const int i = I * kT64 + x, j = J * kT64 + y;
    A[(size_t)i * DP + j] = inside ? val : (i == j ? 1.0 : 0.0);
  });
  if (I == 0 && J == 0 && threadIdx.x == 0) v.c.ctl(t)->reset(0.0);
}

// ---------------------------------------------------------------------------------------------------------------- the quadratic form
// grid (ceil(N / 64), DP / 64, K): rows 64 blockIdx.x .., block column J = DP / 64 - 1 - blockIdx.y, model blockIdx.z
__global__ __launch_bounds__(kWThreads) void scorew_quad_kernel(ScorewIn in, AfterwView v, double* __restrict__ parts) {
  __shared__ __attribute__((aligned(16))) double s_stage[2 * kT64Stage];
  __shared__ double s_half[2][kT64];
  const int DP = v.c.DP, T = DP / kT64, J = T - 1 - (int)blockIdx.y, t = blockIdx.z, j0 = J * kT64;
  const int N = in.N, D = in.D;
  const size_t n0 = (size_t)blockIdx.x * kT64;
  const double* Xt = in.table(t);
  const double* mu = in.mean + (size_t)t * D;
  const double* Pj = v.c.a(t) + (size_t)j0 * DP;  // rows j0 .. of P = its block column J
  auto xc = [&](int x, int k) { return (n0 + x < (size_t)N && k < D) ? Xt[(n0 + x) * D + k] - mu[k] : 0.0; };
  f64x4 acc[2][2];
  t64_zero(acc);
  t64_tile_product<true>(0, j0 + kT64, [&](int which, int x, int k) {
    return which == 0 ? xc(x, k) : (k < j0 ? 2.0 : 1.0) * Pj[(size_t)x * DP + k];
  }, s_stage, s_stage + kT64Stage, acc);
  // e(row, col) = acc(row, col) xc(row, j0 + col) summed over the row: this lane's two columns per (a, r), then the sixteen lanes that
  // share the row (lane bits 0 .. 3), then the two waves that share it
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int l16 = lane & 15, kq = lane >> 4, ri = (w >> 1) * 32, rj = (w & 1) * 32;
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = ri + 16 * a + kq + 4 * r;
      double s = fma(acc[a][1][r], xc(row, j0 + rj + 16 + l16), acc[a][0][r] * xc(row, j0 + rj + l16));
#pragma unroll
      for (int off = 8; off >= 1; off >>= 1) s += __shfl_xor(s, off);
      if (l16 == 0) s_half[w & 1][row] = s;
    }
  __syncthreads();
  if (threadIdx.x < kT64)
    parts[((size_t)t * T + J) * scorew_padded_rows(N) + n0 + threadIdx.x] = s_half[0][threadIdx.x] + s_half[1][threadIdx.x];
}

// ---------------------------------------------------------------------------------------------------------------- logdet P
// grid (K), 256 threads.  Not gated: a flagged model gets NaN.  Kept in the workspace for scorew_finish_kernel; logdet_out may be NULL.
__global__ __launch_bounds__(kWThreads) void scorew_logdet_kernel(int D, AfterwView v, double* __restrict__ logdet_out) {
  __shared__ double s_sum[kWThreads];
  const int t = blockIdx.x, tid = threadIdx.x;
  const bool ok = cholw_gate(v.c.ctl(t));
  const double sum = cholw_log_pivot_sum(v.c, t, D, ok, s_sum);
  if (tid == 0) {
    v.vec(t, AfterwView::kR)[0] = sum;
    if (logdet_out) logdet_out[t] = sum;
  }
}

// ---------------------------------------------------------------------------------------------------------------- q and the log-density
// grid (ceil(N / 256), K): thread = row.  log_density may be NULL (then logdet was not computed and is not read).
__global__ __launch_bounds__(kWThreads) void scorew_finish_kernel(int N, int D, AfterwView v, const double* __restrict__ parts,
                                                                 double* __restrict__ mahalanobis, double* __restrict__ log_density) {
  const int t = blockIdx.y, T = v.c.DP / kT64;
  const size_t n = (size_t)blockIdx.x * kWThreads + threadIdx.x, NP = scorew_padded_rows(N);
  if (n >= (size_t)N) return;
  const double* p = parts + (size_t)t * T * NP + n;
  double q = 0.0;
  for (int J = 0; J < T; ++J) q += p[(size_t)J * NP];
  mahalanobis[(size_t)t * N + n] = q;
  if (log_density) {
    const double logdet = v.vec(t, AfterwView::kR)[0];  // (NaN for a model that is not positive definite)
    log_density[(size_t)t * N + n] = 0.5 * ((logdet - (double)D * 1.8378770664093453) - q);
  }
}

}  // namespace uglad
