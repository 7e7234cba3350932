// The covariance front-end beyond the eigensolver's size (uglad_covariance_wide: every D up to the cell's own limit), fp64 throughout.
// after_path.h's cov_kernel holds a whole table's covariance in one workgroup and repairs it with the one-workgroup eigensolver; neither
// scales past D = 256.  Here a table is spread over many workgroups, and the reference's repair (prepare_data.py:347-352: where the
// smallest eigenvalue is <= 1e-6, S += (offset - min eig) I) needs no eigensolver at all:
//
//   S - sigma I is positive definite  <=>  min eig > sigma,  and a Cholesky factorisation that completes or breaks down decides the left
//   side backward-stably (chol_wide.h, which holds the factorisation, its error bound and the bisection on it).  One factorisation at
//   sigma = 1e-6 takes the reference's decision; for the tables that fail it, 24 bisection steps on [-2^-30 tr S, 1e-6] (CovwBracket; S is a
//   Gram matrix: min eig >= -O(1e-16) tr) bracket the smallest eigenvalue to (1e-6 + 2^-30 tr) / 2^24.  An fp32 inertia count cannot do
//   this: its error ~ sqrt(D) 6e-8 ||S|| is far above the threshold, and a rank-deficient table (N < D, the normal case at these sizes) has
//   min eig ~ 0.
//
//   covw_stats_kernel     per table and block of 64 columns: min, max, mean -> mn, scale, mu (fp64; the semantics of cov_kernel)
//   covw_gram_kernel<Sink>   one workgroup per upper 64 x 64 tile: S = Xc^T Xc / N on the fp64 MFMA, the table streaming through LDS
//                         centred and normalised.  The ONE centred Gram product of the wide utilities: what becomes of an element is its
//                         Sink's.  CovwSink writes the fp64 slab S64 (row stride DP = D rounded up to 64, identity in the padding) and the
//                         fp32 S_out, both triangles (the mirror is a copy: exactly symmetric); eigvals_wide.h has the eigensolver's
//   25 x { cholw_bisect_kernel<CovwBracket>, cholw_update_kernel + cholw_panel_kernel<CholwView> per block column of 64 },
//   cholw_bisect_kernel<CovwBracket>, cholw_repair_kernel
//                         the shift bisection of chol_wide.h (launch_cholw_bisection): the test at the threshold and 24 steps, each a
//                         blocked Cholesky of S64 - sigma I into the slab W; then the diagonals of S64 and S_out += offset - min eig
//
// Every sum has a fixed order (rows over waves combined in wave order, the k-ordered fma chain of the MFMA), so results are bit-reproducible.
// Nothing reads back to the host: the whole sequence (2 + 1 + 25 (2 DP / 64 + 1) + 1 launches) can be captured into a graph.
#pragma once
#include "chol_wide.h"

namespace uglad {

// A table's part of the workspace, in DOUBLES (the buffer is 8-byte aligned; DP = D rounded up to 64), is the factorisation's slab and no more:
//   S64   DP x DP   the covariance in fp64, row stride DP, identity in the padding; repaired in place (CholwView::a)
//   W     DP x DP   the Cholesky factor of S64 - sigma I under test (CholwView::l)
//   mn | scale | mu   3 DP   the column statistics (CholwView::vec3)
//   CholwCtl   8   the bisection's bracket, sigma, min eig and the flags (not PD, active, repaired)
__host__ __device__ constexpr size_t covw_table_doubles(int DP) { return cholw_slab_doubles(DP); }
__host__ inline CholwView covw_view(float* workspace, int D) {
  const int DP = t64_padded(D);
  return CholwView{reinterpret_cast<double*>(workspace), covw_table_doubles(DP), DP};
}
__host__ inline size_t covw_table_floats(int D) { return 2 * covw_table_doubles(t64_padded(D)); }

// the bisection's bracket of a Gram matrix: lower end -2^-30 tr S (the trace of the D x D matrix, lanes striding the diagonal, combined in a
// fixed order)
struct CovwBracket {
  static constexpr int kSteps = 24;  // bisection steps behind the test at the threshold
  __device__ static double lower(const CholwView& v, int t, int D) {
    const double* S64 = v.a(t);
    double tr = 0.0;
    for (int i = (int)threadIdx.x; i < D; i += 64) tr += S64[(size_t)i * v.DP + i];
    return -wave_sum_f64(tr) * (1.0 / 1073741824.0);
  }
};

// ---------------------------------------------------------------------------------------------------------------- column statistics
// grid (DP / 64, K): thread = column (lane) x row group (wave); rows w, w + 4, ...; the four partial results combined in wave order
__global__ __launch_bounds__(kWThreads) void covw_stats_kernel(const double* __restrict__ X, int N, int D, int normalize, CholwView v) {
  __shared__ double s_p[3][4][kT64];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, t = blockIdx.y;
  const int c = blockIdx.x * kT64 + lane;
  const double* Xt = X + (size_t)t * N * D;
  double mn = 1.7976931348623157e308, mx = -1.7976931348623157e308, sm = 0.0;
  bool nan = false;
  if (c < D)
    for (int n = w; n < N; n += 4) {
      const double x = Xt[(size_t)n * D + c];
      nan = nan || (x != x);
      mn = fmin(mn, x);
      mx = fmax(mx, x);
      sm += x;
    }
  s_p[0][w][lane] = nan ? __builtin_nan("") : mn;
  s_p[1][w][lane] = mx;
  s_p[2][w][lane] = sm;
  __syncthreads();
  if (w == 0) {
    mn = s_p[0][0][lane], mx = s_p[1][0][lane], sm = s_p[2][0][lane];
    for (int g = 1; g < 4; ++g) {
      const double a = s_p[0][g][lane];
      mn = (a != a || mn != mn) ? __builtin_nan("") : fmin(mn, a);
      mx = fmax(mx, s_p[1][g][lane]);
      sm += s_p[2][g][lane];
    }
    const double mean = sm / (double)N;
    double* st = v.vec3(t);
    const int cp = blockIdx.x * kT64 + lane;  // (< DP; the padding's statistics are never read)
    if (normalize == 1) {  // (x - min) / (max - min): a constant column gives 0/0 = NaN, as in the reference
      const double sc = 1.0 / (mx - mn);
      st[cp] = mn;
      st[v.DP + cp] = sc;
      st[2 * v.DP + cp] = (mean - mn) * sc;
    } else {
      st[cp] = 0.0;
      st[v.DP + cp] = 1.0;
      st[2 * v.DP + cp] = mean;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- covariance
// grid (DP / 64, DP / 64, K); tiles below the diagonal return.  Ragged N and D are zero-filled AFTER centring.  The statistics are
// covw_stats_kernel's, in vec3 of v's slab (normalize = 0 wrote mn = 0, scale = 1: the loader's (x - 0) * 1 - mu is x - mu to the bit).
// Sink (the caller's): the types View (vec3(t) and DP as CholwView has them) and Out; every thread builds its own as Sink{v, out, D};
//   kSums                       false: cov = S(i, j), the sum / N; true: the centred sum itself (rank_wide.h: exact integers stay exact)
//   put(t, i, j, cov, inside)   per element of the upper triangle of the padded matrix, i <= j < DP; cov = S(i, j) where inside (j < D)
//   finish(t, I, J)             behind the tile's last put, called by the whole workgroup
template <class Sink>
__global__ __launch_bounds__(kWThreads) void covw_gram_kernel(const double* __restrict__ X, int N, int D, typename Sink::View v,
                                                              typename Sink::Out* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) double s_stage[2 * kT64Stage];
  const int I = blockIdx.y, J = blockIdx.x, t = blockIdx.z;
  if (I > J) return;  // (uniform per workgroup)
  const int lane = threadIdx.x & 63, DP = v.DP;
  const double* Xt = X + (size_t)t * N * D;
  const double* st = v.vec3(t);
  // a thread stages the same column of either operand in every chunk (256 = 0 mod 64)
  const int ci = I * kT64 + lane, cj = J * kT64 + lane;
  const double mn[2] = {st[ci], st[cj]}, sc[2] = {st[DP + ci], st[DP + cj]}, mu[2] = {st[2 * DP + ci], st[2 * DP + cj]};
  const int col[2] = {ci, cj};
  f64x4 acc[2][2];
  t64_zero(acc);
  t64_tile_product<false>(0, N, [&](int which, int, int n) {
    return (n < N && col[which] < D) ? (Xt[(size_t)n * D + col[which]] - mn[which]) * sc[which] - mu[which] : 0.0;
  }, s_stage, s_stage + kT64Stage, acc);
  Sink sink{v, out, D};
  t64_for_each_fragment([&](int a, int c, int r, int row, int cl) {
    const int i = I * kT64 + row, j = J * kT64 + cl;
    if (i > j) return;  // (the diagonal tile: its lower half is the mirror of its upper half)
    sink.put(t, i, j, Sink::kSums ? acc[a][c][r] : acc[a][c][r] / (double)N, j < D);  // (i <= j)
  });
  sink.finish(t, I, J);
}

// M(i, j) = val and, where asked, its mirror (a copy: exactly symmetric)
template <class T>
__device__ __forceinline__ void covw_store(T* M, int ld, int i, int j, T val, bool mirror) {
  M[(size_t)i * ld + j] = val;
  if (mirror) M[(size_t)j * ld + i] = val;
}

// the covariance front-end's: the fp64 slab with the identity in the padding, and the fp32 (K, D, D) output
struct CovwSink {
  using View = CholwView;
  using Out = float;
  static constexpr bool kSums = false;
  CholwView v;
  float* S_out;
  int D;
  __device__ void put(int t, int i, int j, double cov, bool inside) const {
    const double val = inside ? cov : (i == j ? 1.0 : 0.0);
    covw_store(v.a(t), v.DP, i, j, val, i != j);
    if (inside) covw_store(S_out + (size_t)t * D * D, D, i, j, (float)val, i != j);
  }
  __device__ void finish(int, int, int) const {}
};

}  // namespace uglad
