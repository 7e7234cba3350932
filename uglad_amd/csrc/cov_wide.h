// The covariance front-end beyond the eigensolver's size (uglad_covariance_wide: every D up to the cell's own limit), fp64 throughout.
// after_path.h's cov_kernel holds a whole table's covariance in one workgroup and repairs it with the one-workgroup eigensolver; neither
// scales past D = 256.  Here a table is spread over many workgroups, and the reference's repair (prepare_data.py:347-352: where the
// smallest eigenvalue is <= 1e-6, S += (offset - min eig) I) needs no eigensolver at all:
//
//   S - sigma I is positive definite  <=>  min eig > sigma,  and a Cholesky factorisation that completes or breaks down decides the left
//   side backward-stably (error <= D (D + 1) 2^-53 ||S||, Higham Thm 10.3).  One factorisation at sigma = 1e-6 takes the reference's
//   decision; for the tables that fail it, 24 bisection steps on [-2^-30 tr S, 1e-6] (S is a Gram matrix: min eig >= -O(1e-16) tr) bracket
//   the smallest eigenvalue to (1e-6 + 2^-30 tr) / 2^24.  An fp32 inertia count cannot do this: its error ~ sqrt(D) 6e-8 ||S|| is far above
//   the threshold, and a rank-deficient table (N < D, the normal case at these sizes) has min eig ~ 0.
//
//   covw_stats_kernel     per table and block of 64 columns: min, max, mean -> mn, scale, mu (fp64; the semantics of cov_kernel)
//   covw_gram_kernel      one workgroup per upper 64 x 64 tile: S = Xc^T Xc / N on the fp64 MFMA, the table streaming through LDS centred
//                         and normalised; writes the fp64 slab S64 (row stride DP = D rounded up to 64, identity in the padding) and the
//                         fp32 S_out, both triangles (the mirror is a copy: exactly symmetric)
//   covw_control_kernel   one workgroup of one wave per table, between two factorisations: reads the "not PD" flag, moves the bracket,
//                         chooses the next sigma
//   covw_chol_update_kernel, covw_chol_panel_kernel
//                         blocked left-looking Cholesky of S64 - sigma I into the slab W, two launches per block column of 64:
//                         A: tile (i, j) = S64(i, j) - sigma delta - sum_{p < j} L(i, p) L(j, p)^T for every i >= j (a tile product, k = 64 j)
//                         B: every workgroup factors the diagonal tile in LDS and solves its own tile against it; the diagonal tile's
//                            workgroup alone raises the flag on a pivot that is <= 0 or NaN (no atomics).  L(j, j) itself is never
//                            stored: no later launch reads it, and the workgroups of THIS launch are still reading the tile it would replace
//                         Every launch returns at once for a table that is flagged or inactive (the gated empties of ns_ldl_phase_kernel).
//                         covw_chol_panel_kernel<true> (after_wide.h, sigma = 0): the diagonal tile's workgroup also runs the solve, on the
//                         identity, and writes L(j, j)^-T and the 64 log-pivots into slabs of their own behind the control block
//   covw_repair_kernel    active tables: the diagonal of S64 += offset - min eig, the diagonal of S_out rewritten from it (one rounding)
//
// Every sum has a fixed order (rows over waves combined in wave order, the k-ordered fma chain of the MFMA), so results are bit-reproducible.
// Nothing reads back to the host: the whole sequence (2 + 1 + 25 (2 DP / 64 + 1) + 1 launches) can be captured into a graph.
#pragma once
#include "wide_ns.h"

namespace uglad {

constexpr int kCovwT = 64;        // tile and block column
constexpr int kCovwK = 32;        // k chunk of the tile products
constexpr int kCovwLd = 80;       // LDS row stride of a [k][x] chunk (as NsTile<64>::kLd)
constexpr int kCovwLdk = kCovwK + 2;  // ... of a [x][k] chunk (as ns_gemm64_kernel's kLdk)
constexpr int kCovwLdt = kCovwT + 1;  // ... of a 64 x 64 tile in the panel kernel
constexpr int kCovwSteps = 24;    // bisection steps behind the test at the threshold
constexpr double kCovwThreshold = 1e-6;  // prepare_data.py:347

// per-table control block, behind the column statistics (8 doubles)
struct CovwCtl {
  double lo, hi, sigma, min_eig;
  int notpd;     // raised by the factorisation of S64 - sigma I
  int active;    // the table failed the test at the threshold: it is being bisected, and will be repaired
  int repaired;  // the repair was applied
  int pad;
};
static_assert(sizeof(CovwCtl) == 48, "the control block fits its 8 doubles");

// what the kernels take: a table's region is `stride` doubles (host_route.h, CovWideLayout)
struct CovwView {
  double* base;   // S64 of table 0
  size_t stride;  // doubles per table
  int DP;
  __host__ __device__ double* s64(int t) const { return base + (size_t)t * stride; }
  __host__ __device__ double* w(int t) const { return s64(t) + (size_t)DP * DP; }
  __host__ __device__ double* stats(int t) const { return w(t) + (size_t)DP * DP; }  // mn | scale | mu, DP each
  __host__ __device__ CovwCtl* ctl(int t) const { return reinterpret_cast<CovwCtl*>(stats(t) + 3 * (size_t)DP); }
  // behind the control block, only in the layout of the factorisation's second client (after_wide.h; covw_chol_panel_kernel<true>):
  // the transposed inverse of the factor, then the logarithms of the DP pivots
  __host__ __device__ double* inv_t(int t) const { return stats(t) + 3 * (size_t)DP + 8; }
  __host__ __device__ double* log_pivot(int t) const { return inv_t(t) + (size_t)DP * DP; }
};
__host__ __device__ constexpr size_t covw_table_doubles(int DP) { return 2 * (size_t)DP * DP + 3 * (size_t)DP + 8; }

// ---------------------------------------------------------------------------------------------------------------- column statistics
// grid (DP / 64, K): thread = column (lane) x row group (wave); rows w, w + 4, ...; the four partial results combined in wave order
__global__ __launch_bounds__(kWThreads) void covw_stats_kernel(const double* __restrict__ X, int N, int D, int normalize, CovwView v) {
  __shared__ double s_p[3][4][kCovwT];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, t = blockIdx.y;
  const int c = blockIdx.x * kCovwT + lane;
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
    double* st = v.stats(t);
    const int cp = blockIdx.x * kCovwT + lane;  // (< DP; the padding's statistics are never read)
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

// ---------------------------------------------------------------------------------------------------------------- the tile product
// acc += sum_k A(x, k) B(y, k) over k0 <= k < k1 on one 64 x 64 tile: four waves, each a 32 x 32 block as 2 x 2 accumulators of
// v_mfma_f64_16x16x4_f64, operand and accumulator layout of ns_gemm64_kernel (lane l supplies A[l & 15][l >> 4], B[l >> 4][l & 15];
// register r of lane l is C[(l >> 4) + 4 r][l & 15]).  Chunks of 32 k go through LDS, the next one prefetched into registers.
// KC = false: the sources run along x (the table: k = row, x = column) and a chunk is kept [k][x];
// KC = true : they run along k (rows of L) and a chunk is kept [x][k].  load(which, x, k) returns the element (zero outside).
template <bool KC, class Load>
__device__ __forceinline__ void covw_tile_product(int k0, int k1, Load&& load, double* sA, double* sB, f64x4 (&acc)[2][2]) {
  constexpr int kPer = kCovwT * kCovwK / kWThreads;  // 8 elements per thread, chunk and operand
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int l16 = lane & 15, kq = lane >> 4, ri = (w >> 1) * 32, rj = (w & 1) * 32;
  double pa[kPer], pb[kPer];
  auto coords = [&](int e, int& x, int& k) {
    const int idx = tid + kWThreads * e;
    if (KC) x = idx >> 5, k = idx & 31;
    else k = idx >> 6, x = idx & 63;
  };
  auto fetch = [&](int kc) {
#pragma unroll
    for (int e = 0; e < kPer; ++e) {
      int x, k;
      coords(e, x, k);
      pa[e] = load(0, x, kc + k);
      pb[e] = load(1, x, kc + k);
    }
  };
  auto stash = [&]() {
#pragma unroll
    for (int e = 0; e < kPer; ++e) {
      int x, k;
      coords(e, x, k);
      const int at = KC ? x * kCovwLdk + k : k * kCovwLd + x;
      sA[at] = pa[e];
      sB[at] = pb[e];
    }
  };
  if (k0 < k1) fetch(k0);
  for (int kc = k0; kc < k1; kc += kCovwK) {
    __syncthreads();  // (the previous chunk has been consumed)
    stash();
    __syncthreads();
    if (kc + kCovwK < k1) fetch(kc + kCovwK);
#pragma unroll
    for (int ks = 0; ks < kCovwK / 4; ++ks) {
      const int k = 4 * ks + kq;
      const double a0 = KC ? sA[(ri + l16) * kCovwLdk + k] : sA[k * kCovwLd + ri + l16];
      const double a1 = KC ? sA[(ri + 16 + l16) * kCovwLdk + k] : sA[k * kCovwLd + ri + 16 + l16];
      const double b0 = KC ? sB[(rj + l16) * kCovwLdk + k] : sB[k * kCovwLd + rj + l16];
      const double b1 = KC ? sB[(rj + 16 + l16) * kCovwLdk + k] : sB[k * kCovwLd + rj + 16 + l16];
      acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
    }
  }
}
constexpr int kCovwStage = kCovwK * kCovwLd;  // doubles per staged operand (>= 64 * kCovwLdk)
static_assert(kCovwT * kCovwLdk <= kCovwStage, "the [x][k] layout fits the operand's staging area");

// ---------------------------------------------------------------------------------------------------------------- covariance
// grid (DP / 64, DP / 64, K); tiles below the diagonal return.  Ragged N and D are zero-filled AFTER centring.
__global__ __launch_bounds__(kWThreads) void covw_gram_kernel(const double* __restrict__ X, int N, int D, CovwView v, float* __restrict__ S_out) {
  __shared__ __attribute__((aligned(16))) double s_stage[2 * kCovwStage];
  const int I = blockIdx.y, J = blockIdx.x, t = blockIdx.z;
  if (I > J) return;  // (uniform per workgroup)
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, DP = v.DP;
  const double* Xt = X + (size_t)t * N * D;
  const double* st = v.stats(t);
  // a thread stages the same column of either operand in every chunk (256 = 0 mod 64)
  const int ci = I * kCovwT + lane, cj = J * kCovwT + lane;
  const double mn[2] = {st[ci], st[cj]}, sc[2] = {st[DP + ci], st[DP + cj]}, mu[2] = {st[2 * DP + ci], st[2 * DP + cj]};
  const int col[2] = {ci, cj};
  f64x4 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int c = 0; c < 2; ++c) acc[a][c] = (f64x4){0.0, 0.0, 0.0, 0.0};
  covw_tile_product<false>(0, N, [&](int which, int, int n) {
    return (n < N && col[which] < D) ? (Xt[(size_t)n * D + col[which]] - mn[which]) * sc[which] - mu[which] : 0.0;
  }, s_stage, s_stage + kCovwStage, acc);
  // ---- epilogue: acc[a][c][r] of lane l = C[ri + 16 a + (l >> 4) + 4 r][rj + 16 c + (l & 15)]
  const int l16 = lane & 15, kq = lane >> 4, ri = (w >> 1) * 32, rj = (w & 1) * 32;
  double* S64 = v.s64(t);
  float* So = S_out + (size_t)t * D * D;
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = I * kCovwT + ri + 16 * a + kq + 4 * r, j = J * kCovwT + rj + 16 * c + l16;
        if (i > j) continue;  // (the diagonal tile: its lower half is the mirror of its upper half)
        const bool inside = j < D;  // (i <= j)
        const double val = inside ? acc[a][c][r] / (double)N : (i == j ? 1.0 : 0.0);  // the padding carries the identity
        S64[(size_t)i * DP + j] = val;
        if (i != j) S64[(size_t)j * DP + i] = val;
        if (inside) {
          So[(size_t)i * D + j] = (float)val;
          if (i != j) So[(size_t)j * D + i] = (float)val;
        }
      }
}

// ---------------------------------------------------------------------------------------------------------------- bisection control
// grid (K), one wave.  step -1: before the first factorisation (sigma = the threshold); step 0: its result -- positive definite there: no
// repair, the table leaves; else the bracket [-2^-30 tr S, threshold]; steps 1 .. kCovwSteps: positive definite => lo = sigma, else hi = sigma.
__global__ __launch_bounds__(64) void covw_control_kernel(int step, int D, CovwView v) {
  const int t = blockIdx.x, lane = threadIdx.x;
  CovwCtl* ctl = v.ctl(t);
  double tr = 0.0;
  if (step == 0) {  // (the trace of the D x D matrix, lanes striding the diagonal, combined in a fixed order)
    const double* S64 = v.s64(t);
    for (int i = lane; i < D; i += 64) tr += S64[(size_t)i * v.DP + i];
    tr = wave_sum_f64(tr);
  }
  if (lane != 0) return;
  if (step < 0) {
    ctl->lo = ctl->hi = ctl->min_eig = 0.0;
    ctl->sigma = kCovwThreshold;
    ctl->notpd = 0, ctl->active = 1, ctl->repaired = 0, ctl->pad = 0;
    return;
  }
  if (!ctl->active) return;
  const bool pd = ctl->notpd == 0;
  if (step == 0) {
    if (pd) {
      ctl->active = 0;
      return;
    }
    ctl->lo = -tr * (1.0 / 1073741824.0);
    ctl->hi = kCovwThreshold;
  } else if (pd) {
    ctl->lo = ctl->sigma;
  } else {
    ctl->hi = ctl->sigma;
  }
  const double mid = 0.5 * (ctl->lo + ctl->hi);
  ctl->sigma = mid;
  ctl->min_eig = mid;  // (after the last step: the estimate)
  ctl->notpd = 0;
}

// a factorisation launch does nothing for a table that left or whose factorisation has broken down; one thread reads, all follow
__device__ __forceinline__ bool covw_gate(const CovwCtl* ctl) {
  __shared__ int s_go;
  if (threadIdx.x == 0) s_go = ctl->active != 0 && ctl->notpd == 0;
  __syncthreads();
  return s_go != 0;
}

// ---------------------------------------------------------------------------------------------------------------- Cholesky, launch A
// grid (DP / 64 - j, K): tile (i, j), i = j + blockIdx.x, of W = S64 - sigma delta - sum_{k < 64 j} L(i, k) L(j, k)
__global__ __launch_bounds__(kWThreads) void covw_chol_update_kernel(int j, CovwView v) {
  __shared__ __attribute__((aligned(16))) double s_stage[2 * kCovwStage];
  const int t = blockIdx.y;
  if (!covw_gate(v.ctl(t))) return;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, DP = v.DP;
  const int i0 = (j + (int)blockIdx.x) * kCovwT, j0 = j * kCovwT;
  const double* S64 = v.s64(t);
  double* W = v.w(t);
  const double* rows[2] = {W + (size_t)i0 * DP, W + (size_t)j0 * DP};
  f64x4 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int c = 0; c < 2; ++c) acc[a][c] = (f64x4){0.0, 0.0, 0.0, 0.0};
  covw_tile_product<true>(0, j0, [&](int which, int x, int k) { return rows[which][(size_t)x * DP + k]; }, s_stage, s_stage + kCovwStage, acc);
  const double sigma = v.ctl(t)->sigma;
  const int l16 = lane & 15, kq = lane >> 4, ri = (w >> 1) * 32, rj = (w & 1) * 32;
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = i0 + ri + 16 * a + kq + 4 * r, jj = j0 + rj + 16 * c + l16;
        const size_t at = (size_t)i * DP + jj;
        W[at] = S64[at] - (i == jj ? sigma : 0.0) - acc[a][c][r];
      }
}

// ---------------------------------------------------------------------------------------------------------------- Cholesky, launch B
// grid (DP / 64 - j, K).  Every workgroup factors the updated diagonal tile (j, j) in LDS -- thread = row (lane) x columns = wave mod 4,
// right-looking, one barrier per column; the column stays unscaled until the end so that every thread forms l_rc = a_rc / sqrt(a_cc) from the
// same bits -- and then solves its own tile X L(j, j)^T = W(i, j) column by column.  A pivot that is <= 0 or NaN ends the factorisation in
// every workgroup alike; the diagonal tile's workgroup raises the flag.  W(j, j) is only read here (all workgroups of the launch load it).
template <bool kKeepDiag>
__global__ __launch_bounds__(kWThreads) void covw_chol_panel_kernel(int j, CovwView v) {
  __shared__ double s_d[kCovwT * kCovwLdt], s_t[kCovwT * kCovwLdt], s_inv[kCovwT];
  const int t = blockIdx.y;
  CovwCtl* ctl = v.ctl(t);
  if (!covw_gate(ctl)) return;
  const int tid = threadIdx.x, r = tid & 63, w = tid >> 6, DP = v.DP;
  const int i0 = (j + (int)blockIdx.x) * kCovwT, j0 = j * kCovwT;
  double* W = v.w(t);
  for (int idx = tid; idx < kCovwT * kCovwT; idx += kWThreads) {
    const int rr = idx >> 6, cc = idx & 63;
    s_d[rr * kCovwLdt + cc] = W[(size_t)(j0 + rr) * DP + j0 + cc];
    s_t[rr * kCovwLdt + cc] = W[(size_t)(i0 + rr) * DP + j0 + cc];
  }
  bool bad = false;
  for (int c = 0; c < kCovwT; ++c) {
    __syncthreads();  // (the loads; the updates of column c - 1)
    const double d = s_d[c * kCovwLdt + c];
    if (!(d > 0.0)) {  // (also NaN; the same bits in every thread of every workgroup)
      bad = true;
      break;
    }
    const double inv = 1.0 / sqrt(d);
    if (tid == 0) s_inv[c] = inv;
    if (r > c) {
      const double lrc = s_d[r * kCovwLdt + c] * inv;
      for (int q = c + 1 + ((w - c - 1) & 3); q <= r; q += 4) s_d[r * kCovwLdt + q] -= lrc * (s_d[q * kCovwLdt + c] * inv);
    }
  }
  if (bad) {
    if (blockIdx.x == 0 && tid == 0) ctl->notpd = 1;
    return;
  }
  const bool diag = blockIdx.x == 0;
  if (diag) {
    if constexpr (!kKeepDiag) return;  // (the diagonal tile's workgroup: its part was the decision)
    // kKeepDiag: the solve below on the identity instead of the tile gives L(j, j)^-T
    for (int idx = tid; idx < kCovwT * kCovwT; idx += kWThreads) s_t[(idx >> 6) * kCovwLdt + (idx & 63)] = (idx >> 6) == (idx & 63) ? 1.0 : 0.0;
  }
  __syncthreads();
  // X L^T = T: x_rc = (t_rc - sum_{p < c} x_rp l_cp) / l_cc, with l_qc = s_d[q][c] inv_c and l_cc = 1 / inv_c
  for (int c = 0; c < kCovwT; ++c) {
    const double inv = s_inv[c];
    if (w == (c & 3)) s_t[r * kCovwLdt + c] *= inv;  // (this thread owns the columns = w mod 4 of row r)
    __syncthreads();
    const double x = s_t[r * kCovwLdt + c];
    for (int q = c + 1 + ((w - c - 1) & 3); q < kCovwT; q += 4) s_t[r * kCovwLdt + q] -= x * (s_d[q * kCovwLdt + c] * inv);
  }
  __syncthreads();
  if constexpr (kKeepDiag) {
    if (diag) {  // into the slab of the inverse, NOT over tile (j, j) of W: the other workgroups of this launch are still reading that
      double* Wt = v.inv_t(t);
      for (int idx = tid; idx < kCovwT * kCovwT; idx += kWThreads) {
        const int rr = idx >> 6, cc = idx & 63;
        Wt[(size_t)(j0 + rr) * DP + j0 + cc] = cc >= rr ? s_t[rr * kCovwLdt + cc] : 0.0;
      }
      if (tid < kCovwT) v.log_pivot(t)[j0 + tid] = log(s_d[tid * kCovwLdt + tid]);
      return;
    }
  }
  for (int idx = tid; idx < kCovwT * kCovwT; idx += kWThreads) {
    const int rr = idx >> 6, cc = idx & 63;
    W[(size_t)(i0 + rr) * DP + j0 + cc] = s_t[rr * kCovwLdt + cc];
  }
}

// ---------------------------------------------------------------------------------------------------------------- repair
// grid (ceil(D / 256), K): S += (eval_offset - min eig) I for the tables that failed the test at the threshold; min_eig_out[t] = the
// smallest eigenvalue before the repair, or +infinity for a table that passed (its eigenvalue is never computed)
__global__ __launch_bounds__(256) void covw_repair_kernel(int D, double eval_offset, CovwView v, float* __restrict__ S_out,
                                                          double* __restrict__ min_eig_out) {
  const int t = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  CovwCtl* ctl = v.ctl(t);
  const bool active = ctl->active != 0;
  const double mn = ctl->min_eig;
  if (active && i < D) {
    double* S64 = v.s64(t);
    const double d = S64[(size_t)i * v.DP + i] + (eval_offset - mn);
    S64[(size_t)i * v.DP + i] = d;
    S_out[(size_t)t * D * D + (size_t)i * D + i] = (float)d;
  }
  if (i == 0) {
    min_eig_out[t] = active ? mn : __builtin_inf();
    ctl->repaired = active ? 1 : 0;
  }
}

}  // namespace uglad
