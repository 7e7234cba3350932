// The available-case (pairwise-complete) covariance of a table with missing entries (uglad_pairwise_covariance; additive: the reference
// fills every NaN with the column mean, main.py:647-670, which shrinks the variances by about (1 - p) and the off-diagonals by about
// (1 - p)^2 at a missing fraction p), fp64 throughout, on the tile layer of chol_wide.h, and the reference's repair
// (prepare_data.py:347-352) for a matrix that is NOT a Gram matrix.  What pandas' DataFrame.cov and R's cov(use = "pairwise.complete.obs")
// compute, with the reference's divisor.
//
// Only NaN counts as missing.  For a table X (N x D), with m_ni = 1 where x_ni is observed, mn_i / mx_i the observed minimum / maximum of
// column i, y = (x - mn_i) * (1 / (mx_i - mn_i)) under normalize = 1 and y = x otherwise, mu_i the mean of the observed y_.i and
// z_ni = m_ni (y_ni - mu_i):
//
//   n_ij = sum_n m_ni m_nj      a_ij = sum_n z_ni m_nj      p_ij = sum_n z_ni z_nj
//   cov_ij = p_ij / n_ij - (a_ij / n_ij) (a_ji / n_ij)
//
// the covariance of the rows where both columns are observed, every mean taken over those rows, divided by n_ij (as the reference's
// empirical_covariance divides by N; pandas' cov is this times n_ij / (n_ij - 1)).  The shift by mu_i changes nothing mathematically: it
// keeps a column offset from cancelling catastrophically in p - a a / n.  Which rounding of the observed mean serves as mu_i is the
// implementation's: here (sum of the observed x, rows over waves, / count - mn) * scale, the host formulation's the mean of the observed
// y; the two differ by rounding and so do the results, within the tests' bound.  Two calls of THIS implementation give the same bits.
//
//   pairw_stats_kernel    per table and block of 64 columns: observed count, minimum, maximum, mean (rows over waves, combined in wave order)
//                         -> mn, scale, mu in vec3, as covw_stats_kernel leaves them, and the column's flag word
//   pairw_gram_kernel     one workgroup per upper 64 x 64 tile: in ONE pass over the table the four products n = Mi^T Mj, a = Zi^T Mj,
//                         b = Mi^T Zj (= a_ji: no second tile is read), p = Zi^T Zj on the fp64 MFMA.  LDS holds what covw_gram_kernel's
//                         holds: the chunk of y - mu with NaN kept (ragged rows and columns staged as NaN); m = (v == v) and z = m ? v : 0
//                         are made in registers at the operand read: 16 MFMA per k-step of 4.  The four accumulator sets take 128
//                         AGPR next to 234 VGPR (no spills): ONE workgroup per compute unit where covw_gram_kernel runs two, so the
//                         loads of a chunk are hidden by the register prefetch alone (profiles/pairwise_probe.txt has the measured
//                         ratio of the two kernels).  Then cov per element of the upper
//                         triangle, the mirror a copy, into the fp64 slab (identity in the padding), S_out and the optional outputs
//   pairw_info_kernel     the flag words -> info_out, and their OR per table
//   assoc_rowsum_kernel, the shift bisection of chol_wide.h on AssocBracket: the matrix is in general INDEFINITE (every entry has its own
//                         set of rows), so cov_wide.h's bracket of a Gram matrix would not hold its smallest eigenvalue
//   pairw_bar_kernel      a table with any flag set holds NaN: behind the controller's reset it leaves the bisection (CholwCtl::active = 0,
//                         what cholw_gate reads: every launch of the 49 factorisations returns at once for it, and it cannot touch its
//                         neighbours' bits); behind the repair its min_eig_out becomes NaN
//
// Flags (int32 per column): 1 the column has no observed entry; 2 the column is in a pair with fewer than min_pairs jointly observed rows
// (that entry is NaN; a pair with a column flagged 1, 4 or 8 does not count: the partner's flag says it all); 4 normalize = 1 and the
// observed values are constant (0 / 0, as the reference's NaN); 8 the column holds an infinity -- a value, not a missing entry: it
// propagates as it does on the host, NaN in the column's row and column.  Bit 8 is this implementation's addition to the three flags the
// front-end was specified with: without it the propagated NaN would run through the 49 factorisations unannounced; with it the table is
// barred from the repair like any flagged one.  A column flagged 1, 4 or 8 has NaN in its row and column.
//
// Every sum has a fixed order (rows over waves combined in wave order, the k-ordered fma chain of the MFMA); the only atomics are integer
// ORs of flag bits.  Nothing reads back to the host.
#pragma once
#include "assoc_wide.h"

namespace uglad {

constexpr int kPairwEmpty = 1, kPairwFewPairs = 2, kPairwConstant = 4, kPairwInfinite = 8;
constexpr int kPairwDead = kPairwEmpty | kPairwConstant | kPairwInfinite;  // the column's row and column are NaN

// A table's part of the workspace, in DOUBLES: the factorisation's slab (chol_wide.h; A = the covariance, vec3 = mn | scale | mu and, for
// the bisection, the absolute row sums over mn) and behind it DP + 2 int32: the columns' flag words, their OR, one unused.
struct PairwView {
  CholwView c;
  __host__ __device__ int* flags(int t) const { return reinterpret_cast<int*>(c.a(t) + cholw_slab_doubles(c.DP)); }
  __host__ __device__ int* table_flags(int t) const { return flags(t) + c.DP; }
};
__host__ __device__ constexpr size_t pairw_table_doubles(int DP) { return cholw_slab_doubles(DP) + (size_t)DP / 2 + 1; }
__host__ inline PairwView pairw_view(float* workspace, int D) {
  const int DP = t64_padded(D);
  return PairwView{CholwView{reinterpret_cast<double*>(workspace), pairw_table_doubles(DP), DP}};
}
__host__ inline size_t pairw_table_floats(int D) { return 2 * pairw_table_doubles(t64_padded(D)); }

// ---------------------------------------------------------------------------------------------------------------- column statistics
// grid (DP / 64, K): thread = column (lane) x row group (wave); rows w, w + 4, ...; the four partial results combined in wave order.
// A flagged column is staged as it is (mn = 0, scale = 1, mu = 0): its counts stay exact, and whatever its products hold is confined to
// its row and column, which the Gram kernel's finish overwrites with NaN.
__global__ __launch_bounds__(kWThreads) void pairw_stats_kernel(const double* __restrict__ X, int N, int D, int normalize, PairwView v) {
  __shared__ double s_p[4][4][kT64];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, t = blockIdx.y;
  const int c = blockIdx.x * kT64 + lane;  // (< DP)
  const double* Xt = X + (size_t)t * N * D;
  double cnt = 0.0, mn = __builtin_inf(), mx = -__builtin_inf(), sm = 0.0;
  if (c < D)
    for (int n = w; n < N; n += 4) {
      const double x = Xt[(size_t)n * D + c];
      if (x == x) {
        cnt += 1.0;
        mn = fmin(mn, x);
        mx = fmax(mx, x);
        sm += x;
      }
    }
  s_p[0][w][lane] = cnt;
  s_p[1][w][lane] = mn;
  s_p[2][w][lane] = mx;
  s_p[3][w][lane] = sm;
  __syncthreads();
  if (w != 0) return;
  cnt = s_p[0][0][lane], mn = s_p[1][0][lane], mx = s_p[2][0][lane], sm = s_p[3][0][lane];
  for (int g = 1; g < 4; ++g) {
    cnt += s_p[0][g][lane];
    mn = fmin(mn, s_p[1][g][lane]);
    mx = fmax(mx, s_p[2][g][lane]);
    sm += s_p[3][g][lane];
  }
  int flag = 0;
  if (c < D) {
    if (cnt == 0.0) flag = kPairwEmpty;
    else if (mn == -__builtin_inf() || mx == __builtin_inf()) flag = kPairwInfinite;
    else if (normalize == 1 && mx == mn) flag = kPairwConstant;
  }
  const bool plain = flag != 0 || c >= D;
  const double mean = plain ? 0.0 : sm / cnt;
  double* st = v.c.vec3(t);
  const int DP = v.c.DP;
  if (normalize == 1 && !plain) {
    const double sc = 1.0 / (mx - mn);
    st[c] = mn;
    st[DP + c] = sc;
    st[2 * DP + c] = (mean - mn) * sc;
  } else {  // (the loader's (x - 0) * 1 - mu is x - mu to the bit)
    st[c] = 0.0;
    st[DP + c] = 1.0;
    st[2 * DP + c] = mean;
  }
  v.flags(t)[c] = flag;
}

// ---------------------------------------------------------------------------------------------------------------- the four tile products
// acc[0] += Ma^T Mb, acc[1] += Za^T Mb, acc[2] += Ma^T Zb, acc[3] += Za^T Zb over the rows 0 <= k < N of two blocks of 64 columns of a
// table: t64_tile_product<false>'s staging layout ([k][x] chunks of 32 rows, the next one prefetched into registers) and fragment map, ONE
// pass and one staged value per cell -- v = load(which, k), NaN for a missing cell and outside the table -- from which the operand read
// makes m = (v == v) and z = m ? v : 0.  load(which, k) returns column `lane` of block `which` in row k: a thread stages the same column
// in every chunk (256 = 0 mod 64).
template <class Load>
__device__ __forceinline__ void pairw_tile_products(int N, Load&& load, double* sA, double* sB, f64x4 (&acc)[4][2][2]) {
  constexpr int kPer = kT64 * kT64K / kWThreads;  // 8 rows per thread, chunk and operand
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int l16 = lane & 15, kq = lane >> 4, ri = (w >> 1) * 32, rj = (w & 1) * 32;
  double pa[kPer], pb[kPer];
  auto fetch = [&](int kc) {
#pragma unroll
    for (int e = 0; e < kPer; ++e) {
      pa[e] = load(0, kc + w + 4 * e);
      pb[e] = load(1, kc + w + 4 * e);
    }
  };
  fetch(0);
  for (int kc = 0; kc < N; kc += kT64K) {
    __syncthreads();  // (the previous chunk has been consumed)
#pragma unroll
    for (int e = 0; e < kPer; ++e) {
      sA[(w + 4 * e) * kT64Ld + lane] = pa[e];
      sB[(w + 4 * e) * kT64Ld + lane] = pb[e];
    }
    __syncthreads();
    if (kc + kT64K < N) fetch(kc + kT64K);
#pragma unroll
    for (int ks = 0; ks < kT64K / 4; ++ks) {
      const int k = 4 * ks + kq;
      const double va[2] = {sA[k * kT64Ld + ri + l16], sA[k * kT64Ld + ri + 16 + l16]};
      const double vb[2] = {sB[k * kT64Ld + rj + l16], sB[k * kT64Ld + rj + 16 + l16]};
      double ma[2], za[2], mb[2], zb[2];
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        ma[q] = va[q] == va[q] ? 1.0 : 0.0;
        za[q] = va[q] == va[q] ? va[q] : 0.0;
        mb[q] = vb[q] == vb[q] ? 1.0 : 0.0;
        zb[q] = vb[q] == vb[q] ? vb[q] : 0.0;
      }
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          acc[0][a][c] = __builtin_amdgcn_mfma_f64_16x16x4f64(ma[a], mb[c], acc[0][a][c], 0, 0, 0);
          acc[1][a][c] = __builtin_amdgcn_mfma_f64_16x16x4f64(za[a], mb[c], acc[1][a][c], 0, 0, 0);
          acc[2][a][c] = __builtin_amdgcn_mfma_f64_16x16x4f64(ma[a], zb[c], acc[2][a][c], 0, 0, 0);
          acc[3][a][c] = __builtin_amdgcn_mfma_f64_16x16x4f64(za[a], zb[c], acc[3][a][c], 0, 0, 0);
        }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- covariance
// the optional outputs of uglad_pairwise_covariance, each NULL or (K, D, D)
struct PairwOut {
  float* S;        // fp32, never NULL
  double* S64;     // fp64, unrepaired
  int* counts;     // n_ij
};

// grid (DP / 64, DP / 64, K); tiles below the diagonal return.  The statistics and the flags 1, 4, 8 are pairw_stats_kernel's.
__global__ __launch_bounds__(kWThreads) void pairw_gram_kernel(const double* __restrict__ X, int N, int D, int min_pairs, PairwView v,
                                                               PairwOut out) {
  __shared__ __attribute__((aligned(16))) double s_stage[2 * kT64Stage];
  const int I = blockIdx.y, J = blockIdx.x, t = blockIdx.z;
  if (I > J) return;  // (uniform per workgroup)
  const int lane = threadIdx.x & 63, DP = v.c.DP;
  const double* Xt = X + (size_t)t * N * D;
  const double* st = v.c.vec3(t);
  const int col[2] = {I * kT64 + lane, J * kT64 + lane};
  const double mn[2] = {st[col[0]], st[col[1]]}, sc[2] = {st[DP + col[0]], st[DP + col[1]]}, mu[2] = {st[2 * DP + col[0]], st[2 * DP + col[1]]};
  f64x4 acc[4][2][2];
#pragma unroll
  for (int q = 0; q < 4; ++q) t64_zero(acc[q]);
  pairw_tile_products(N, [&](int which, int n) {
    return (n < N && col[which] < D) ? (Xt[(size_t)n * D + col[which]] - mn[which]) * sc[which] - mu[which] : __builtin_nan("");
  }, s_stage, s_stage + kT64Stage, acc);
  int* flags = v.flags(t);
  double* S64 = v.c.a(t);
  const size_t base = (size_t)t * D * D;
  const double need = (double)min_pairs;
  t64_for_each_fragment([&](int a, int c, int r, int row, int cl) {
    const int i = I * kT64 + row, j = J * kT64 + cl;
    if (i > j) return;  // (the diagonal tile: its lower half is the mirror of its upper half)
    const bool mirror = i != j;
    if (j >= D) {  // (i <= j: the padding carries the identity)
      covw_store(S64, DP, i, j, i == j ? 1.0 : 0.0, mirror);
      return;
    }
    const double n = acc[0][a][c][r], aij = acc[1][a][c][r], aji = acc[2][a][c][r], p = acc[3][a][c][r];
    const bool dead = ((flags[i] | flags[j]) & kPairwDead) != 0, few = n < need;
    if (few && !dead) {
      atomicOr(flags + i, kPairwFewPairs);
      atomicOr(flags + j, kPairwFewPairs);
    }
    const double val = (dead || few) ? __builtin_nan("") : p / n - (aij / n) * (aji / n);
    covw_store(S64, DP, i, j, val, mirror);
    covw_store(out.S + base, D, i, j, (float)val, mirror);
    if (out.S64) covw_store(out.S64 + base, D, i, j, val, mirror);
    if (out.counts) covw_store(out.counts + base, D, i, j, (int)n, mirror);
  });
}

// ---------------------------------------------------------------------------------------------------------------- flags
// grid (K): the columns' flag words -> info_out (K, D) or NULL; their OR -> table_flags (an OR: any order gives the same bits)
__global__ __launch_bounds__(kWThreads) void pairw_info_kernel(int D, PairwView v, int* __restrict__ info_out) {
  __shared__ int s_any[kWThreads];
  const int t = blockIdx.x, tid = threadIdx.x;
  const int* flags = v.flags(t);
  int any = 0;
  for (int c = tid; c < D; c += kWThreads) {
    const int f = flags[c];
    if (info_out) info_out[(size_t)t * D + c] = f;
    any |= f;
  }
  s_any[tid] = any;
  __syncthreads();
  if (tid == 0) {
    for (int k = 1; k < kWThreads; ++k) any |= s_any[k];
    *v.table_flags(t) = any;
  }
}

// grid (K), one thread.  after_repair = 0, behind the controller's reset: a flagged table leaves the bisection; 1, behind the repair: its
// min_eig_out is NaN (cholw_repair_kernel wrote +infinity, as for every table that is not repaired)
__global__ __launch_bounds__(64) void pairw_bar_kernel(int after_repair, PairwView v, double* __restrict__ min_eig_out) {
  const int t = blockIdx.x;
  if (threadIdx.x != 0 || *v.table_flags(t) == 0) return;
  if (after_repair) min_eig_out[t] = __builtin_nan("");
  else v.c.ctl(t)->active = 0;
}

}  // namespace uglad
