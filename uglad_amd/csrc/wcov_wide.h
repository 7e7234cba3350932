// The covariances of ONE table under R weightings of its rows (uglad_weighted_covariance; additive: the reference has no resampling), fp64
// throughout, on the tile layer of chol_wide.h, and the reference's repair (prepare_data.py:347-352) as cov_wide.h runs it.  A bootstrap
// resample is a weighting by integer multiplicities, a subsample or a cross-validation fold one by 0 / 1, a kernel-smoothed window one by
// real weights: the table goes to the device once, and one staged chunk of it feeds several weightings' accumulators.
//
// For a table X (N x D) and the weights w_n >= 0 of weighting r, with s = sum_n w_n and mu = sum_n w_n x_n / s:
//
//   S = sum_n w_n (x_n - mu) (x_n - mu)^T / s
//
// -- empirical_covariance of the table with row n repeated w_n times, for integer weights.  Sharing a staged chunk needs a centring that
// does not depend on the weighting, so the table is shifted by its UNWEIGHTED column means c and the weighting's own centre comes in at
// the end:  G = sum_n w_n (x_n - c) (x_n - c)^T,  d = sum_n w_n (x_n - c) / s = mu - c,  S = G / s - d d^T.  For resamples of one table d is
// O(sigma / sqrt(N)) and by Cauchy-Schwarz |d_i d_j| <= sqrt(G_ii G_jj) / s always: the subtraction costs a few ulps of sqrt(G_ii G_jj) / s,
// the scale the Gram sum's own rounding has.  d is summed from the shifted values, so a column offset cancels in x - c and nowhere else.
//
//   covw_stats_kernel     (cov_wide.h) on X as a single table: c, into vec3 of slab 0 -- what the weightings share
//   wcov_stats_kernel     per weighting and block of 64 columns: s, d, mu and the flag word (rows over waves, combined in wave order)
//   wcov_gram_kernel<G>   one workgroup per upper 64 x 64 tile and group of G weightings: t64_weighted_tile_products -- the chunk of
//                         x - c staged once, the chunk's weights next to it, w a formed in registers, G accumulator sets f64x4[2][2];
//                         then G / s - d d^T per element of the upper triangle, the mirror a copy, into the weighting's fp64 slab
//                         (identity in the padding), S_out and S64_out.  A last group with fewer than G weightings stages zero weights
//                         for the missing ones and writes nothing for them
//   the shift bisection of chol_wide.h on CovwBracket over K = R slabs: a weighted Gram matrix with w >= 0 is positive semi-definite up
//                         to rounding, as the covariance is
//   wcov_bar_kernel       a flagged weighting holds NaN: behind the controller's reset it leaves the bisection, behind the repair its
//                         min_eig_out becomes NaN (pairwise_wide.h's pairw_bar_kernel, on this view)
//
// Flags (int32 per weighting): 1 a weight is negative, NaN or infinite; 2 the weights sum to zero.  A flagged weighting is NaN throughout.
//
// Every sum has a fixed order (rows over waves combined in wave order, the k-ordered fma chain of the MFMA); no atomics.  A weighting's
// bits depend on the table and on its own weights alone: not on R, not on its place in the call or in its group.  Nothing reads back to
// the host.
#pragma once
#include "cov_wide.h"

namespace uglad {

constexpr int kWcovGroup = 4;  // weightings per workgroup of the Gram kernel: 4 x 32 AGPR of accumulators (pairwise_wide.h runs the same four)
constexpr int kWcovBadWeight = 1, kWcovZeroSum = 2;

// A weighting's part of the workspace, in DOUBLES: the factorisation's slab (chol_wide.h; A = the covariance; vec3 of slab 0 holds the
// table's mn = 0 | scale = 1 | c as covw_stats_kernel leaves them for a single table, the other slabs' vec3 stays unused) and behind it
//   d      DP    mu - c, zero in the padding
//   s      1     the sum of the weights
//   flag   1     the flag word (int32, and one unused)
struct WcovView {
  CholwView c;
  __host__ __device__ double* shift(int r) const { return c.a(r) + cholw_slab_doubles(c.DP); }
  __host__ __device__ double* sum(int r) const { return shift(r) + c.DP; }
  __host__ __device__ int* flag(int r) const { return reinterpret_cast<int*>(sum(r) + 1); }
  __host__ __device__ double* table_mean() const { return c.vec3(0) + 2 * (size_t)c.DP; }
};
__host__ __device__ constexpr size_t wcov_weighting_doubles(int DP) { return cholw_slab_doubles(DP) + (size_t)DP + 2; }
__host__ inline WcovView wcov_view(float* workspace, int D) {
  const int DP = t64_padded(D);
  return WcovView{CholwView{reinterpret_cast<double*>(workspace), wcov_weighting_doubles(DP), DP}};
}
__host__ inline size_t wcov_weighting_floats(int D) { return 2 * wcov_weighting_doubles(t64_padded(D)); }

// the optional outputs of uglad_weighted_covariance
struct WcovOut {
  float* S;       // (R, D, D) fp32, never NULL
  double* S64;    // (R, D, D) fp64 or NULL, unrepaired
  double* mean;   // (R, D) or NULL
  int* info;      // (R,), never NULL
};

// ---------------------------------------------------------------------------------------------------------------- the weighting's sums
// grid (DP / 64, R): thread = column (lane) x row group (wave); rows w, w + 4, ...; the four partial results combined in wave order.  Every
// column's thread sums the weights in the same order, so s has the same bits in every workgroup of a weighting; block 0 publishes it.
__global__ __launch_bounds__(kWThreads) void wcov_stats_kernel(const double* __restrict__ X, const double* __restrict__ W, int N, int D,
                                                               WcovView v, WcovOut out) {
  __shared__ double s_s[4][kT64], s_x[4][kT64];
  __shared__ int s_bad[4];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = blockIdx.y;
  const int c = blockIdx.x * kT64 + lane;  // (< DP)
  const double* Wr = W + (size_t)r * N;
  const double cm = v.table_mean()[c];
  double sw = 0.0, sx = 0.0;
  int bad = 0;
  for (int n = w; n < N; n += 4) {
    const double wn = Wr[n];
    bad |= (!(wn >= 0.0) || wn == __builtin_inf()) ? 1 : 0;  // (also NaN)
    sw += wn;
    if (c < D) sx += wn * (X[(size_t)n * D + c] - cm);
  }
  if (lane == 0) s_bad[w] = bad;
  const double s = t64_sum_waves(sw, s_s);
  const double x = t64_sum_waves(sx, s_x);
  if (w != 0) return;
  int flag = (s_bad[0] | s_bad[1] | s_bad[2] | s_bad[3]) ? kWcovBadWeight : 0;
  if (s == 0.0) flag |= kWcovZeroSum;
  const double d = flag ? __builtin_nan("") : x / s;
  v.shift(r)[c] = c < D ? d : 0.0;
  if (out.mean && c < D) out.mean[(size_t)r * D + c] = flag ? __builtin_nan("") : cm + d;
  if (blockIdx.x == 0 && lane == 0) {
    *v.sum(r) = s;
    v.flag(r)[0] = flag;
    v.flag(r)[1] = 0;
    out.info[r] = flag;
  }
}

// ---------------------------------------------------------------------------------------------------------------- covariance
// grid (DP / 64, DP / 64, ceil(R / G)); tiles below the diagonal return.  Ragged N and D are zero-filled AFTER the shift.  c, s, d and the
// flags are the two statistics kernels'.
template <int G>
__global__ __launch_bounds__(kWThreads) void wcov_gram_kernel(const double* __restrict__ X, const double* __restrict__ W, int R, int N, int D,
                                                              WcovView v, WcovOut out) {
  __shared__ __attribute__((aligned(16))) double s_stage[2 * kT64Stage];
  __shared__ double s_w[G * kT64K];
  const int I = blockIdx.y, J = blockIdx.x, r0 = blockIdx.z * G;
  if (I > J) return;  // (uniform per workgroup)
  const int lane = threadIdx.x & 63, DP = v.c.DP;
  // a thread stages the same column of either operand in every chunk (256 = 0 mod 64)
  const int col[2] = {I * kT64 + lane, J * kT64 + lane};
  const double* mean = v.table_mean();
  const double cm[2] = {mean[col[0]], mean[col[1]]};
  f64x4 acc[G][2][2];
#pragma unroll
  for (int g = 0; g < G; ++g) t64_zero(acc[g]);
  t64_weighted_tile_products<G>(
      N, [&](int which, int, int n) { return (n < N && col[which] < D) ? X[(size_t)n * D + col[which]] - cm[which] : 0.0; },
      [&](int g, int n) { return (r0 + g < R && n < N) ? W[(size_t)(r0 + g) * N + n] : 0.0; }, s_stage, s_stage + kT64Stage, s_w, acc);
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const int r = r0 + g;
    if (r >= R) continue;  // (uniform per workgroup) the ragged last group
    const double s = *v.sum(r);
    const bool bad = v.flag(r)[0] != 0;
    const double* d = v.shift(r);
    double* S64 = v.c.a(r);
    const size_t base = (size_t)r * D * D;
    // a lane's sixteen elements lie in eight rows and two columns: their d, loaded together ahead of the stores (zero in the padding)
    double di[2][4], dj[2];
    t64_for_each_fragment([&](int a, int c, int q, int row, int cl) {
      if (c == 0) di[a][q] = d[I * kT64 + row];
      if (a == 0 && q == 0) dj[c] = d[J * kT64 + cl];
    });
    t64_for_each_fragment([&](int a, int c, int q, int row, int cl) {
      const int i = I * kT64 + row, j = J * kT64 + cl;
      if (i > j) return;  // (the diagonal tile: its lower half is the mirror of its upper half)
      const bool mirror = i != j;
      if (j >= D) {  // (i <= j: the padding carries the identity)
        covw_store(S64, DP, i, j, i == j ? 1.0 : 0.0, mirror);
        return;
      }
      const double val = bad ? __builtin_nan("") : acc[g][a][c][q] / s - di[a][q] * dj[c];
      covw_store(S64, DP, i, j, val, mirror);
      covw_store(out.S + base, D, i, j, (float)val, mirror);
      if (out.S64) covw_store(out.S64 + base, D, i, j, val, mirror);
    });
  }
}

// grid (R), one thread.  after_repair = 0, behind the controller's reset: a flagged weighting leaves the bisection (CholwCtl::active = 0,
// what cholw_gate reads); 1, behind the repair: its min_eig_out is NaN (cholw_repair_kernel wrote +infinity, as for every slab that is not
// repaired)
__global__ __launch_bounds__(64) void wcov_bar_kernel(int after_repair, WcovView v, double* __restrict__ min_eig_out) {
  const int r = blockIdx.x;
  if (threadIdx.x != 0 || v.flag(r)[0] == 0) return;
  if (after_repair) min_eig_out[r] = __builtin_nan("");
  else v.c.ctl(r)->active = 0;
}

}  // namespace uglad
