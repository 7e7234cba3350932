// All eigenvalues of K symmetric fp64 matrices, 1 <= D <= the cell's own limit (uglad_eigvalsh_wide, uglad_table_spectrum), values only, many
// workgroups per matrix.  The one-workgroup eigensolver (eig_lean.h) stops at D = 256; beyond it the package had the smallest eigenvalue
// alone, from a chain of Cholesky factorisations (chol_wide.h).  The matrix solved is the symmetric part (A + A^T) / 2, as score_wide.h
// takes P.
//
// Stage 1, Householder tridiagonalisation Q^T A Q = T in ONE stage, blocked in panels of 64 columns (LAPACK's dsytrd / dlatrd, lower form).
// Both triangles of A are kept, exactly symmetric, so that "column j" is row j and the matrix-vector product reads whole 64-row strips.
//   eigw_prepare_kernel   one workgroup per tile: (A + A^T) / 2 (chol_wide.h's t64_symmetric_part) into the slab (row stride DP = D
//                         rounded up to 64, ZERO in the padding: every reflector is zero there, so the padding never takes part) and the
//                         tile's "holds a non-finite entry" flag
//   covw_gram_kernel<EigwGramSink>   (uglad_table_spectrum) the same slab from a table: cov_wide.h's centred Gram product / N, optionally
//                         also written out as the (K, D, D) fp64 covariance
//   per column j:
//     eigw_column_kernel  one workgroup per slab.  First it finishes column j - 1: y = the strip partials of A v summed in strip order,
//                         w = tau (y - tau/2 (y^T v) v).  Then column j: row j with the panel's pending corrections applied
//                         (a = A[j][j:] - sum_q V_q w_q[j] + W_q v_q[j]; all but the last reflector's were applied by the launch before),
//                         d_j = a_j, the reflector of a[j+1:] (e_j = beta; a tail that is exactly zero gives tau = 0), v into the panel's V,
//                         and g = W^T v, h = V^T v over the panel's earlier reflectors -- the one part of dlatrd's corrections that needs
//                         a reduction over the rows, and the only pass over the panel that one workgroup makes
//     eigw_matvec_kernel  grid (column chunks of 256, strips of 64 rows, K): partial[s][k] = sum_{i in strip s} A[i][k] v_i, rows in order; the
//                         strips and chunks left of column j + 1 are not launched.  The first strip's workgroups also spread dlatrd's
//                         corrections over the columns, one pass over V and W: partial -= V g + W h, and the next column's
//                         row j + 1 - sum_{q < p} V_q w_q[j + 1] + W_q v_q[j + 1]
//   per panel:
//     eigw_update_kernel  A -= V W^T + W V^T on the trailing matrix: one tile product of k = 128 per UPPER 64 x 64 tile (t64_tile_product on
//                         v_mfma_f64_16x16x4_f64), the mirror tile written from the same values
// Stage 2, the eigenvalues of T by Sturm-count bisection:
//   eigw_bisect_kernel    one thread per eigenvalue index, d and e^2 in LDS, the bracket from Gershgorin's discs widened as dstebz does, the
//                         pivot of the recurrence clamped to -pivmin (a select, no branch), kEigwSteps steps -- a compile-time count
//   eigw_summary_kernel   per slab: min, max, min |.|, max |.|, con = max |.| / min |.| (the reference's condition number,
//                         prepare_data.py:323-325) and the number of eigenvalues < th
//
// Launches: 2 D + D / 64 + 3, each depending on the one before; the 2 D small ones are where the time goes, the
// MFMA work is below 25 GFLOP at D = 2048.
// No loop anywhere depends on the data, so a NaN or Inf cannot spin: a slab that holds one returns NaN in all D places (the flags of
// eigw_prepare_kernel; a d or e that overflowed on the way counts too).  Every sum has a fixed order and there are no floating-point
// atomics: the bits are reproducible and a slab's result does not depend on its neighbours in the batch.  Index m of the output bisects
// for the m-th eigenvalue from the same first bracket as every other index; where two indices part, the smaller one takes the lower half.
// So the output is ascending whatever the rounding of the counts.
#pragma once
#include "cov_wide.h"

namespace uglad {

constexpr int kEigwPanel = kT64;   // columns per panel = the tile edge
constexpr int kEigwChunk = 256;    // columns per workgroup of the matrix-vector product
constexpr int kEigwSteps = 62;     // bisection steps: the bracket (<= 2.2 ||T||) shrinks below 2^-60 ||T||
constexpr int kEigwSummary = 6;    // doubles per slab of the summary: min, max, min |.|, max |.|, con, count below th
static_assert(kWThreads == kEigwChunk && kWThreads == 4 * kT64, "thread = column of a chunk; wave = a quarter of a panel's reflectors");

struct EigwCtl {
  double tau;  // of the reflector under way
  double pad[7];
};

// A slab of the workspace, in DOUBLES (DP = t64_padded(D), nt = DP / 64).  It begins like the factorisation's (CholwView: A, a second DP x DP
// area, three vectors, a control block of 8), so that cov_wide.h's column statistics serve uglad_table_spectrum unchanged:
//   A      DP x DP    the matrix, both triangles; tridiagonalised in place
//   R      DP x DP    scratch: the strip partials of A v (nt x DP), behind them the nt x nt tile flags (ints); from behind_flags(t) on
//                     it is a client's (corr_wide.h), at least kEigwSpare doubles
//   vec3   3 DP       (table entry) mn | scale | mu of covw_stats_kernel
//   EigwCtl   8
//   V | W  64 x DP each   the panel's reflectors and their w, one per row, zero outside (j, D)
//   d | e  DP each    the tridiagonal
//   g | h  64 each    W_q^T v and V_q^T v of the reflector under way, q < its place in the panel
//   arow   DP         row j + 1 with the corrections of the reflectors before column j applied (made next to A v_j, used by column j + 1)
struct EigwView {
  double* base;
  size_t stride;
  int DP;
  __host__ __device__ double* a(int t) const { return base + (size_t)t * stride; }
  __host__ __device__ double* r(int t) const { return a(t) + (size_t)DP * DP; }
  __host__ __device__ int* flags(int t) const { return reinterpret_cast<int*>(r(t) + (size_t)(DP / kT64) * DP); }
  __host__ __device__ double* behind_flags(int t) const { return r(t) + (size_t)(DP / kT64) * DP + (size_t)(DP / kT64) * (DP / kT64); }
  __host__ __device__ double* vec3(int t) const { return r(t) + (size_t)DP * DP; }
  __host__ __device__ EigwCtl* ctl(int t) const { return reinterpret_cast<EigwCtl*>(vec3(t) + 3 * (size_t)DP); }
  __host__ __device__ double* V(int t) const { return vec3(t) + 3 * (size_t)DP + 8; }
  __host__ __device__ double* W(int t) const { return V(t) + (size_t)kEigwPanel * DP; }
  __host__ __device__ double* d(int t) const { return W(t) + (size_t)kEigwPanel * DP; }
  __host__ __device__ double* e(int t) const { return d(t) + DP; }
  __host__ __device__ double* gh(int t) const { return e(t) + DP; }
  __host__ __device__ double* arow(int t) const { return gh(t) + 2 * kEigwPanel; }
  __host__ __device__ CholwView chol() const { return CholwView{base, stride, DP}; }
};
static_assert(sizeof(EigwCtl) == 64, "the control block is the factorisation's 8 doubles");
// the doubles of R from behind_flags(t) on: DP^2 - nt DP - nt^2 (nt^2 doubles cover the nt^2 ints) = nt^2 kEigwSpare, least at nt = 1
constexpr size_t kEigwSpare = (size_t)kT64 * kT64 - kT64 - 1;
__host__ __device__ constexpr size_t eigw_slab_doubles(int DP) { return cholw_slab_doubles(DP) + (2 * (size_t)kEigwPanel + 3) * DP + 2 * kEigwPanel; }
__host__ inline size_t eigw_slab_floats(int D) { return 2 * eigw_slab_doubles(t64_padded(D)); }
__host__ inline EigwView eigw_view(float* workspace, int D) {
  const int DP = t64_padded(D);
  return EigwView{reinterpret_cast<double*>(workspace), eigw_slab_doubles(DP), DP};
}

// the sum of one value per thread, the same bits in every thread: 16 sums of 16 in thread order, then their sum in order.  s_buf: 272 doubles.
// The first barrier protects s_buf's previous use.
__device__ __forceinline__ double eigw_block_sum(double part, double* s_buf) {
  const int tid = threadIdx.x;
  __syncthreads();
  s_buf[tid] = part;
  __syncthreads();
  if (tid < 16) {
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < 16; ++k) s += s_buf[16 * tid + k];
    s_buf[kWThreads + tid] = s;
  }
  __syncthreads();
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < 16; ++k) s += s_buf[kWThreads + k];
  return s;
}
__device__ __forceinline__ bool eigw_finite(double x) { return x - x == 0.0; }
// the workgroup's "some thread saw a non-finite value", written by thread 0 to *flag
__device__ __forceinline__ void eigw_raise(bool bad, int* flag, int* flag_mirror) {
  __shared__ int s_bad;
  if (threadIdx.x == 0) s_bad = 0;
  __syncthreads();
  if (bad) s_bad = 1;  // (every writer stores the same value)
  __syncthreads();
  if (threadIdx.x == 0) *flag = *flag_mirror = s_bad;
}

// ---------------------------------------------------------------------------------------------------------------- the slab
// grid (DP / 64, DP / 64, K): tile (I, J) = (blockIdx.y, blockIdx.x) of (A + A^T) / 2, which is zero in the padding
__global__ __launch_bounds__(kWThreads) void eigw_prepare_kernel(const double* __restrict__ A_in, int D, EigwView v) {
  const int I = blockIdx.y, J = blockIdx.x, t = blockIdx.z, DP = v.DP, nt = DP / kT64;
  double* A = v.a(t);
  bool bad = false;
  t64_symmetric_part(A_in + (size_t)t * D * D, D, I, J, [&](int x, int y, double val, bool) {
    bad = bad || !eigw_finite(val);
    A[(size_t)(I * kT64 + x) * DP + J * kT64 + y] = val;
  });
  int* f = v.flags(t);
  eigw_raise(bad, f + I * nt + J, f + I * nt + J);
}

// covw_gram_kernel's sink for the slab of a table's covariance: zero in the padding, the mirror always written (the diagonal twice), the
// flags of the tile and of its mirror; cov_out: (K, D, D) fp64 or NULL
struct EigwGramSink {
  using View = EigwView;
  using Out = double;
  static constexpr bool kSums = false;
  EigwView v;
  double* cov_out;
  int D;
  bool bad = false;  // this thread put a non-finite value
  __device__ void put(int t, int i, int j, double cov, bool inside) {
    const double val = inside ? cov : 0.0;
    bad = bad || !eigw_finite(val);
    covw_store(v.a(t), v.DP, i, j, val, true);
    if (inside && cov_out) covw_store(cov_out + (size_t)t * D * D, D, i, j, val, true);
  }
  __device__ void finish(int t, int I, int J) const {
    const int nt = v.DP / kT64;
    int* f = v.flags(t);
    eigw_raise(bad, f + I * nt + J, f + J * nt + I);
  }
};

// ---------------------------------------------------------------------------------------------------------------- one column
// grid (K), one workgroup per slab: finishes the reflector of column jprev (>= 0), then starts column j (>= 0)
__global__ __launch_bounds__(kWThreads) void eigw_column_kernel(int jprev, int j, int D, EigwView v) {
  __shared__ double s_y[kNsMaxD];
  __shared__ double s_part[kT64 * kT64Ldt];  // (>= 272: also eigw_block_sum's buffer)
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, t = blockIdx.x, DP = v.DP, nt = DP / kT64;
  double* V = v.V(t);
  double* W = v.W(t);
  if (jprev >= 0) {  // y = the strip partials in strip order (the panel's corrections are in the first strip's); w = tau (y - tau/2 (y^T v) v)
    const int p = jprev & (kEigwPanel - 1), s0 = (jprev + 1) / kT64;
    const double tau = v.ctl(t)->tau;
    const double* vrow = V + (size_t)p * DP;
    const double* R = v.r(t);
    double part = 0.0;
    for (int i = tid; i < DP; i += kWThreads) {
      double y = 0.0;
      if (i > jprev && i < D) {
        for (int s = s0; s < nt; ++s) y += R[(size_t)s * DP + i];
        part = fma(y, vrow[i], part);
      }
      s_y[i] = y;
    }
    const double yv = eigw_block_sum(part, s_part);
    const double alpha = -0.5 * tau * (tau * yv);
    double* wrow = W + (size_t)p * DP;
    for (int i = tid; i < DP; i += kWThreads) wrow[i] = (i > jprev && i < D) ? fma(alpha, vrow[i], tau * s_y[i]) : 0.0;
    __syncthreads();  // (the workgroup's own stores to W, read below)
  }
  if (j < 0) return;
  // column j = row j: the panel's first from A; a later one from arow (the reflectors before column j - 1, eigw_matvec_kernel) and the last reflector
  const int p = j & (kEigwPanel - 1);
  const double* src = p == 0 ? v.a(t) + (size_t)j * DP : v.arow(t);
  const double* vlast = V + (size_t)(p > 0 ? p - 1 : 0) * DP;
  const double* wlast = W + (size_t)(p > 0 ? p - 1 : 0) * DP;
  const double vj = p > 0 ? vlast[j] : 0.0, wj = p > 0 ? wlast[j] : 0.0;
  double part = 0.0;
  for (int i = tid; i < DP; i += kWThreads) {
    double a = 0.0;
    if (i >= j && i < D) {
      a = src[i];
      if (p > 0) {
        a = fma(-vlast[i], wj, a);
        a = fma(-wlast[i], vj, a);
      }
      if (i >= j + 2) part = fma(a, a, part);
    }
    s_y[i] = a;
  }
  const double ss = eigw_block_sum(part, s_part);  // (its barriers also publish s_y)
  const double dj = s_y[j];
  if (j > D - 2) {  // the last column: its diagonal element alone
    if (tid == 0) v.d(t)[j] = dj, v.e(t)[j] = 0.0;
    return;
  }
  const double alpha = s_y[j + 1];
  const double norm = sqrt(fma(alpha, alpha, ss));
  const bool trivial = ss == 0.0;  // (also an exactly tridiagonal or diagonal matrix; NaN is not trivial and spreads)
  const double beta = trivial ? alpha : (alpha >= 0.0 ? -norm : norm);
  const double tau = trivial ? 0.0 : (beta - alpha) / beta;
  const double scale = trivial ? 0.0 : 1.0 / (alpha - beta);
  double* vrow = V + (size_t)p * DP;
  __syncthreads();  // (every thread has read s_y[j] and s_y[j + 1]; s_y now takes v)
  for (int i = tid; i < DP; i += kWThreads) {
    const double vi = i == j + 1 ? 1.0 : ((i >= j + 2 && i < D) ? s_y[i] * scale : 0.0);
    vrow[i] = vi;
    s_y[i] = vi;
  }
  if (tid == 0) {
    v.d(t)[j] = dj;
    v.e(t)[j] = beta;
    v.ctl(t)->tau = tau;
  }
  if (p == 0) return;  // (uniform) no earlier reflector in this panel
  __syncthreads();
  // g_q = W_q^T v (kind 0), h_q = V_q^T v (kind 1), q < p: wave w keeps the reflectors q = w mod 4, a lane the elements i = lane mod 64; a
  // lane's partial sums go through LDS and are added in lane order
  for (int kind = 0; kind < 2; ++kind) {
    const double* Mx = kind == 0 ? W : V;
    double acc[kEigwPanel / 4];
#pragma unroll
    for (int qq = 0; qq < kEigwPanel / 4; ++qq) acc[qq] = 0.0;
    for (int i = (j + 1) / kT64 * kT64 + lane; i < D; i += kT64) {
      const double vi = s_y[i];  // (zero up to j)
#pragma unroll
      for (int qq = 0; qq < kEigwPanel / 4; ++qq) {
        const int q = 4 * qq + w;
        if (q < p) acc[qq] = fma(Mx[(size_t)q * DP + i], vi, acc[qq]);
      }
    }
    __syncthreads();  // (s_part's previous use)
#pragma unroll
    for (int qq = 0; qq < kEigwPanel / 4; ++qq) s_part[(4 * qq + w) * kT64Ldt + lane] = acc[qq];
    __syncthreads();
    if (tid < kT64) {
      double sum = 0.0;
      for (int l = 0; l < kT64; ++l) sum += s_part[tid * kT64Ldt + l];
      v.gh(t)[kind * kEigwPanel + tid] = sum;
    }
  }
}

// grid (chunks from column j + 1 on, strips from row j + 1 on, K): partial[s][k] = sum_{i in strip s} A[i][k] v_i.  The first strip's workgroups
// also take the panel's pending corrections off their columns, one pass over V and W: partial -= V g + W h (dlatrd; g, h from
// eigw_column_kernel), and arow[k] = A[j + 1][k] - sum_{q < p} V_q[k] W_q[j + 1] + W_q[k] V_q[j + 1] for the next column of the same panel
__global__ __launch_bounds__(kWThreads) void eigw_matvec_kernel(int j, EigwView v) {
  __shared__ double s_v[kT64];
  __shared__ double s_q[4][kT64];  // g, h, W_q[j + 1], V_q[j + 1]
  const int tid = threadIdx.x, t = blockIdx.z, DP = v.DP, p = j & (kEigwPanel - 1);
  const int s = (j + 1) / kT64 + (int)blockIdx.y, k = ((j + 1) / kEigwChunk + (int)blockIdx.x) * kEigwChunk + tid;
  const bool first = blockIdx.y == 0;  // (uniform per workgroup)
  const double* V = v.V(t);
  const double* W = v.W(t);
  if (tid < kT64) s_v[tid] = V[(size_t)p * DP + s * kT64 + tid];
  if (first) {
    const int q = tid & (kT64 - 1), which = tid >> 6;
    s_q[which][q] = q >= p ? 0.0 : (which < 2 ? v.gh(t)[which * kEigwPanel + q] : (which == 2 ? W : V)[(size_t)q * DP + j + 1]);
  }
  __syncthreads();
  if (k >= DP) return;
  const double* A = v.a(t) + (size_t)s * kT64 * DP + k;
  double acc = 0.0;
#pragma unroll 16
  for (int r = 0; r < kT64; ++r) acc = fma(A[(size_t)r * DP], s_v[r], acc);
  if (first) {
    double a = v.a(t)[(size_t)(j + 1) * DP + k];
    for (int q = 0; q < p; ++q) {
      const double vq = V[(size_t)q * DP + k], wq = W[(size_t)q * DP + k];
      acc = fma(-vq, s_q[0][q], acc);
      acc = fma(-wq, s_q[1][q], acc);
      a = fma(-vq, s_q[2][q], a);
      a = fma(-wq, s_q[3][q], a);
    }
    v.arow(t)[k] = a;
  }
  v.r(t)[(size_t)s * DP + k] = acc;
}

// grid (T, T, K), T = the tiles behind the panel that starts at column j0: tile (I, J), I <= J, of A -= V W^T + W V^T, and its mirror
__global__ __launch_bounds__(kWThreads) void eigw_update_kernel(int j0, EigwView v) {
  __shared__ __attribute__((aligned(16))) double s_stage[2 * kT64Stage];
  const int I = blockIdx.y, J = blockIdx.x, t = blockIdx.z;
  if (I > J) return;  // (uniform per workgroup)
  const int DP = v.DP, first = j0 / kT64 + 1;
  const int i0 = (first + I) * kT64, c0 = (first + J) * kT64;
  const double* V = v.V(t);
  const double* W = v.W(t);
  f64x4 acc[2][2];
  t64_zero(acc);
  t64_tile_product<false>(0, 2 * kEigwPanel, [&](int which, int x, int k) {
    const int q = k & (kEigwPanel - 1);
    const bool takes_v = (k < kEigwPanel) == (which == 0);  // rows: V then W; columns: W then V
    return (takes_v ? V : W)[(size_t)q * DP + (which == 0 ? i0 : c0) + x];
  }, s_stage, s_stage + kT64Stage, acc);
  double* A = v.a(t);
  t64_for_each_fragment([&](int a, int c, int r, int row, int cl) {
    const int i = i0 + row, k = c0 + cl;
    if (i > k) return;  // (the diagonal tile)
    const double val = A[(size_t)i * DP + k] - acc[a][c][r];
    A[(size_t)i * DP + k] = val;
    A[(size_t)k * DP + i] = val;
  });
}

// ---------------------------------------------------------------------------------------------------------------- the tridiagonal's eigenvalues
// grid (ceil(D / 256), K): thread = eigenvalue index; every workgroup stages the whole of d and e^2 and forms the same bracket
__global__ __launch_bounds__(kWThreads) void eigw_bisect_kernel(int D, EigwView v, double* __restrict__ eig_out) {
  __shared__ double s_d[kNsMaxD], s_e2[kNsMaxD];
  __shared__ double s_red[4][kWThreads];
  const int tid = threadIdx.x, t = blockIdx.y, nt = v.DP / kT64;
  const double* d = v.d(t);
  const double* e = v.e(t);
  const int* flags = v.flags(t);
  double gl = 1.7976931348623157e308, gu = -1.7976931348623157e308, emax2 = 0.0, poison = 0.0;
  for (int i = tid; i < nt * nt; i += kWThreads) poison += flags[i] ? __builtin_nan("") : 0.0;
  for (int i = tid; i < D; i += kWThreads) {
    const double di = d[i], ea = i + 1 < D ? fabs(e[i]) : 0.0, eb = i > 0 ? fabs(e[i - 1]) : 0.0;
    s_d[i] = di;
    s_e2[i] = ea * ea;
    gl = fmin(gl, di - ea - eb);
    gu = fmax(gu, di + ea + eb);
    emax2 = fmax(emax2, ea * ea);
    poison += 0.0 * di + 0.0 * (ea * ea);  // NaN for a d or e that is not finite
  }
  s_red[0][tid] = gl, s_red[1][tid] = gu, s_red[2][tid] = emax2, s_red[3][tid] = poison;
  __syncthreads();
  for (int k = 0; k < kWThreads; ++k) {  // (every thread the same sweep: the same bits)
    gl = fmin(gl, s_red[0][k]);
    gu = fmax(gu, s_red[1][k]);
    emax2 = fmax(emax2, s_red[2][k]);
    poison += s_red[3][k];
  }
  const int m = blockIdx.x * kWThreads + tid;
  if (m >= D) return;
  // dstebz: pivmin = safe minimum * max(1, max e^2); the discs widened by 2.1 ||T|| ulp D + 2.1 pivmin on either side
  const double pivmin = 2.2250738585072014e-308 * fmax(1.0, emax2);
  const double bnorm = fmax(fabs(gl), fabs(gu)), widen = 2.1 * bnorm * 2.220446049250313e-16 * (double)D + 2.1 * 2.0 * pivmin;
  double lo = gl - widen, hi = gu + widen;
  for (int step = 0; step < kEigwSteps; ++step) {
    const double mid = lo + 0.5 * (hi - lo);
    int count = 0;  // the eigenvalues of T below mid
    double q = 1.0;
    for (int i = 0; i < D; ++i) {
      q = s_d[i] - mid - (i > 0 ? s_e2[i - 1] / q : 0.0);
      q = fabs(q) < pivmin ? -pivmin : q;
      count += q < 0.0 ? 1 : 0;
    }
    const bool below = count <= m;  // the m-th eigenvalue (from 0) is >= mid
    lo = below ? mid : lo;
    hi = below ? hi : mid;
  }
  const double val = gl == gu ? gl : lo + 0.5 * (hi - lo);  // (discs of one point: T = gl I, e.g. the zero matrix -- exactly, not to pivmin)
  eig_out[(size_t)t * D + m] = poison == 0.0 ? val : __builtin_nan("");
}

// grid (K): the summary of a slab's eigenvalues (ascending, or all NaN)
__global__ __launch_bounds__(kWThreads) void eigw_summary_kernel(int D, double th, const double* __restrict__ eig, double* __restrict__ summary) {
  __shared__ double s_red[2][kWThreads];
  __shared__ int s_cnt[kWThreads];
  const int tid = threadIdx.x, t = blockIdx.x;
  const double* ev = eig + (size_t)t * D;
  double mn = 1.7976931348623157e308, mx = 0.0;
  int cnt = 0;
  for (int i = tid; i < D; i += kWThreads) {
    const double a = fabs(ev[i]);
    mn = fmin(mn, a);
    mx = fmax(mx, a);
    cnt += ev[i] < th ? 1 : 0;
  }
  s_red[0][tid] = mn, s_red[1][tid] = mx, s_cnt[tid] = cnt;
  __syncthreads();
  if (tid != 0) return;
  for (int k = 1; k < kWThreads; ++k) {
    mn = fmin(mn, s_red[0][k]);
    mx = fmax(mx, s_red[1][k]);
    cnt += s_cnt[k];
  }
  const bool nan = ev[0] != ev[0];  // (a slab is NaN in all places or in none)
  double* out = summary + (size_t)t * kEigwSummary;
  out[0] = ev[0];
  out[1] = ev[D - 1];
  out[2] = nan ? ev[0] : mn;
  out[3] = nan ? ev[0] : mx;
  out[4] = nan ? ev[0] : mx / mn;
  out[5] = (double)cnt;
}

}  // namespace uglad
