// What the many-workgroup fp64 utilities stand on (cov_wide.h, assoc_wide.h, after_wide.h, score_wide.h, eigvals_wide.h): the 64 x 64 tile layer on
// v_mfma_f64_16x16x4_f64, the blocked Cholesky factorisation of a slab that is spread over many workgroups, and the bisection of a slab's
// smallest eigenvalue on that factorisation.
//
// The tile layer (t64_): a workgroup of 256 threads owns one 64 x 64 tile; each of its four waves owns a 32 x 32 quadrant as 2 x 2 accumulators
// f64x4.  The lane-to-element layout of those accumulators is written down ONCE, in t64_for_each_fragment; t64_zero clears them,
// t64_tile_product fills them (t64_weighted_tile_products: several sets from one staged chunk; both on t64_tile_sweep, which holds the
// staging once), t64_for_each_element is the plain (row, column) sweep of a tile that goes to or from LDS, and
// t64_symmetric_part is a tile of (A + A^T) / 2, symmetric to the bit, for the clients that take a matrix as it was fitted.
//
// The factorisation (cholw_): A - sigma I = L L^T, blocked left-looking on 64 x 64 tiles, two launches per block column j:
//   cholw_update_kernel   tile (i, j) = A(i, j) - sigma delta - sum_{p < j} L(i, p) L(j, p)^T for every i >= j (a tile product, k = 64 j)
//   cholw_panel_kernel    every workgroup factors the diagonal tile in LDS and solves its own tile against it; the diagonal tile's workgroup
//                         alone raises the flag on a pivot that is <= 0 or NaN (no atomics)
// Whether the factorisation completes or breaks down decides "A - sigma I is positive definite" backward-stably (error <= D (D + 1) 2^-53
// ||A||, Higham Thm 10.3) and without pivoting, since nothing past the first bad pivot is used.  Every launch returns at once for a slab that
// is flagged or inactive (cholw_gate), so a sequence of factorisations needs no readback.
// L(j, j) itself is never stored over tile (j, j): no later launch of the factorisation reads it, and the other workgroups of the SAME panel
// launch are still reading the tile it would replace.  A client that needs the diagonal factor asks for its inverse instead: on a
// CholwInvView the diagonal tile's workgroup also runs the panel's solve on the identity and writes L(j, j)^-T and the 64 log-pivots into
// slabs of their own behind the control block.  Only a layout that has those slabs can make that view (after_wide.h); a CholwView cannot
// reach the code that writes them.
//
//
// The shift bisection (cholw_bisect_kernel, cholw_repair_kernel): the reference's repair (prepare_data.py:347-352: where the smallest eigenvalue
// is <= 1e-6, A += (offset - min eig) I) from factorisations alone.  One at sigma = the threshold takes the reference's decision; for the slabs
// that fail it, Bracket::kSteps bisection steps on [Bracket::lower, threshold] bracket the smallest eigenvalue.  The client owns the Bracket
// (where its matrix's smallest eigenvalue cannot lie below, and how many steps that bracket needs); the controller and the repair are here.
//
// Every sum has a fixed order (the k-ordered fma chain of the MFMA, columns in index order), so results are bit-reproducible.
#pragma once
#include "wide_ns.h"

namespace uglad {

constexpr int kT64 = 64;            // tile and block column
constexpr int kT64K = 32;           // k chunk of the tile products
constexpr int kT64Ld = 80;          // LDS row stride of a [k][x] chunk (as NsTile<64>::kLd)
constexpr int kT64Ldk = kT64K + 2;  // ... of a [x][k] chunk (as ns_gemm64_kernel's kLdk)
constexpr int kT64Ldt = kT64 + 1;   // ... of a 64 x 64 tile kept whole
constexpr int kT64Stage = kT64K * kT64Ld;  // doubles per staged operand (>= 64 * kT64Ldk)
static_assert(kT64 * kT64Ldk <= kT64Stage, "the [x][k] layout fits the operand's staging area");
__host__ __device__ constexpr int t64_padded(int D) { return (D + kT64 - 1) / kT64 * kT64; }  // DP: D rounded up to whole tiles

// ---------------------------------------------------------------------------------------------------------------- the fragment map
// Wave w of the workgroup owns rows ri = 32 (w >> 1) .., columns rj = 32 (w & 1) .. of the tile; acc[a][c][r] of lane l is
// C[ri + 16 a + (l >> 4) + 4 r][rj + 16 c + (l & 15)] (the accumulator layout of v_mfma_f64_16x16x4_f64, as in ns_gemm64_kernel).
// Calls f(a, c, r, row, col) for the calling lane's sixteen elements, row and col inside the tile; fully unrolled.
template <class F>
__device__ __forceinline__ void t64_for_each_fragment(F&& f) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int l16 = lane & 15, kq = lane >> 4, ri = (w >> 1) * 32, rj = (w & 1) * 32;
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int r = 0; r < 4; ++r) f(a, c, r, ri + 16 * a + kq + 4 * r, rj + 16 * c + l16);
}
__device__ __forceinline__ void t64_zero(f64x4 (&acc)[2][2]) {
  acc[0][0] = acc[0][1] = acc[1][0] = acc[1][1] = (f64x4){0.0, 0.0, 0.0, 0.0};
}
// f(row, col) for every element of the tile, the workgroup's threads striding it in row-major order
template <class F>
__device__ __forceinline__ void t64_for_each_element(F&& f) {
  for (int idx = threadIdx.x; idx < kT64 * kT64; idx += kWThreads) f(idx >> 6, idx & 63);
}
// thread = element (lane) x group (wave) of a 64-wide row: the four waves' partial sums of element `lane`, combined in wave order -- the same
// bits in the four waves.  One barrier, behind the stores; a caller that uses s_part again puts its own barrier in front of that.
__device__ __forceinline__ double t64_sum_waves(double part, double (&s_part)[4][kT64]) {
  const int lane = threadIdx.x & 63;
  s_part[threadIdx.x >> 6][lane] = part;
  __syncthreads();
  return ((s_part[0][lane] + s_part[1][lane]) + s_part[2][lane]) + s_part[3][lane];
}

// tile (I, J) of (A + A^T) / 2 of a (D, D) fp64 matrix: tiles (I, J) and (J, I) of A go through LDS (zero outside the matrix; one barrier),
// then f(x, y, value, inside) for every element of the tile as t64_for_each_element deals them; inside: row 64 I + x and column 64 J + y
// are both < D (value is zero elsewhere).  Called by the whole workgroup, once per kernel.
template <class F>
__device__ __forceinline__ void t64_symmetric_part(const double* __restrict__ A, int D, int I, int J, F&& f) {
  __shared__ double s_a[kT64 * kT64Ldt], s_b[kT64 * kT64Ldt];
  const int i0 = I * kT64, j0 = J * kT64;
  t64_for_each_element([&](int a, int b) {
    s_a[a * kT64Ldt + b] = (i0 + a < D && j0 + b < D) ? A[(size_t)(i0 + a) * D + j0 + b] : 0.0;
    s_b[a * kT64Ldt + b] = (j0 + a < D && i0 + b < D) ? A[(size_t)(j0 + a) * D + i0 + b] : 0.0;
  });
  __syncthreads();
  t64_for_each_element([&](int x, int y) { f(x, y, 0.5 * (s_a[x * kT64Ldt + y] + s_b[y * kT64Ldt + x]), i0 + x < D && j0 + y < D); });
}

// ---------------------------------------------------------------------------------------------------------------- the tile product
// The sweep of the tile products over k0 <= k < k1: the operand layout of ns_gemm64_kernel (lane l supplies A[l & 15][l >> 4],
// B[l >> 4][l & 15]).  Chunks of 32 k go through LDS, the next one prefetched into registers.
// KC = false: the sources run along x (a table: k = row, x = column) and a chunk is kept [k][x];
// KC = true : they run along k (rows of L) and a chunk is kept [x][k].  load(which, x, k) returns the element (zero outside).
// What a product adds to the chunk: fetch_more(kc) next to the prefetch of the chunk at kc, stash_more() next to its stores into LDS
// (between the two barriers); what it does with the operands: step(k, a0, a1, b0, b1) per k-step of 4, k = this lane's k inside the
// chunk, a0 / a1 and b0 / b1 the lane's operand elements of the wave's two row and two column blocks of 16.
template <bool KC, class Load, class FetchMore, class StashMore, class Step>
__device__ __forceinline__ void t64_tile_sweep(int k0, int k1, Load&& load, double* sA, double* sB, FetchMore&& fetch_more,
                                               StashMore&& stash_more, Step&& step) {
  constexpr int kPer = kT64 * kT64K / kWThreads;  // 8 elements per thread, chunk and operand
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
    fetch_more(kc);
  };
  auto stash = [&]() {
#pragma unroll
    for (int e = 0; e < kPer; ++e) {
      int x, k;
      coords(e, x, k);
      const int at = KC ? x * kT64Ldk + k : k * kT64Ld + x;
      sA[at] = pa[e];
      sB[at] = pb[e];
    }
    stash_more();
  };
  if (k0 < k1) fetch(k0);
  for (int kc = k0; kc < k1; kc += kT64K) {
    __syncthreads();  // (the previous chunk has been consumed)
    stash();
    __syncthreads();
    if (kc + kT64K < k1) fetch(kc + kT64K);
#pragma unroll
    for (int ks = 0; ks < kT64K / 4; ++ks) {
      const int k = 4 * ks + kq;
      const double a0 = KC ? sA[(ri + l16) * kT64Ldk + k] : sA[k * kT64Ld + ri + l16];
      const double a1 = KC ? sA[(ri + 16 + l16) * kT64Ldk + k] : sA[k * kT64Ld + ri + 16 + l16];
      const double b0 = KC ? sB[(rj + l16) * kT64Ldk + k] : sB[k * kT64Ld + rj + l16];
      const double b1 = KC ? sB[(rj + 16 + l16) * kT64Ldk + k] : sB[k * kT64Ld + rj + 16 + l16];
      step(k, a0, a1, b0, b1);
    }
  }
}

// acc += sum_k A(x, k) B(y, k) over k0 <= k < k1 on one 64 x 64 tile, the accumulators as above
template <bool KC, class Load>
__device__ __forceinline__ void t64_tile_product(int k0, int k1, Load&& load, double* sA, double* sB, f64x4 (&acc)[2][2]) {
  t64_tile_sweep<KC>(k0, k1, load, sA, sB, [](int) {}, [] {}, [&](int, double a0, double a1, double b0, double b1) {
    acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
    acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
    acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
    acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
  });
}

// acc[g] += sum_k w_g(k) A(x, k) B(y, k) over the rows 0 <= k < N of two blocks of 64 columns of a table, for G weightings of its rows at
// once: ONE staged chunk of the two operands (KC = false) feeds G accumulator sets, the chunk's G x 32 weights staged next to it in sW
// (G * kT64K doubles; thread t < 32 G stages weight(t / 32, k) of row k = t mod 32).  The weight goes into ONE operand fragment, in
// registers (no square root: w a is exact for a 0 / 1 weight); weight(g, k) returns 0 outside the table and for a weighting that is not
// there.  A weighting's sums do not depend on g or on its neighbours.  Each set costs 32 accumulator registers (pairwise_wide.h).
template <int G, class Load, class Weight>
__device__ __forceinline__ void t64_weighted_tile_products(int N, Load&& load, Weight&& weight, double* sA, double* sB, double* sW,
                                                           f64x4 (&acc)[G][2][2]) {
  static_assert(G * kT64K <= kWThreads, "one thread per staged weight");
  const int tid = threadIdx.x;
  double pw = 0.0;
  t64_tile_sweep<false>(
      0, N, load, sA, sB,
      [&](int kc) {
        if (tid < G * kT64K) pw = weight(tid / kT64K, kc + tid % kT64K);
      },
      [&] {
        if (tid < G * kT64K) sW[tid] = pw;
      },
      [&](int k, double a0, double a1, double b0, double b1) {
#pragma unroll
        for (int g = 0; g < G; ++g) {
          const double wk = sW[g * kT64K + k], wa0 = wk * a0, wa1 = wk * a1;
          acc[g][0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(wa0, b0, acc[g][0][0], 0, 0, 0);
          acc[g][0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(wa0, b1, acc[g][0][1], 0, 0, 0);
          acc[g][1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(wa1, b0, acc[g][1][0], 0, 0, 0);
          acc[g][1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(wa1, b1, acc[g][1][1], 0, 0, 0);
        }
      });
}

// ---------------------------------------------------------------------------------------------------------------- control block and views
// One per slab (8 doubles of the workspace).  The factorisation reads sigma, notpd and active; the rest is the bisection's (below).
struct CholwCtl {
  double lo, hi;   // (bisection) the bracket of the smallest eigenvalue
  double sigma;    // the shift of the factorisation under way
  double min_eig;  // (bisection) the estimate
  int notpd;       // raised by the factorisation of A - sigma I
  int active;      // the slab is still being factored; bisection: it failed the test at the threshold and will be repaired
  int repaired;    // (bisection) the repair was applied
  int pad;
  __device__ void reset(double s) {
    lo = hi = min_eig = 0.0;
    sigma = s;
    notpd = 0, active = 1, repaired = 0, pad = 0;
  }
};
static_assert(sizeof(CholwCtl) == 48, "the control block fits its 8 doubles");

// What the factorisation's kernels take.  Slab t is `stride` doubles; it begins with (DP = t64_padded(D), row stride DP)
//   A     DP x DP   the matrix, identity in the padding
//   L     DP x DP   the factor of A - sigma I: the tiles below the block diagonal (the diagonal tiles stay unfactored)
//   vec3  3 DP      three vectors of the client's
//   CholwCtl   8
// and goes on as its client's layout says.
struct CholwView {
  static constexpr bool kKeepsInverse = false;
  double* base;   // A of slab 0
  size_t stride;  // doubles per slab
  int DP;
  __host__ __device__ double* a(int t) const { return base + (size_t)t * stride; }
  __host__ __device__ double* l(int t) const { return a(t) + (size_t)DP * DP; }
  __host__ __device__ double* vec3(int t) const { return l(t) + (size_t)DP * DP; }
  __host__ __device__ CholwCtl* ctl(int t) const { return reinterpret_cast<CholwCtl*>(vec3(t) + 3 * (size_t)DP); }
};
__host__ __device__ constexpr size_t cholw_slab_doubles(int DP) { return 2 * (size_t)DP * DP + 3 * (size_t)DP + 8; }

// ... of a layout that goes on, behind the control block, with Wt = L^-T (DP x DP, block upper triangular) and the logarithms of the DP
// pivots.  No data of its own: the kernels' argument block is CholwView's.  Made by afterw_view alone.
struct AfterwView;
struct CholwInvView : CholwView {
  static constexpr bool kKeepsInverse = true;
  __host__ __device__ double* inv_t(int t) const { return vec3(t) + 3 * (size_t)DP + 8; }
  __host__ __device__ double* log_pivot(int t) const { return inv_t(t) + (size_t)DP * DP; }

 private:
  __host__ __device__ explicit CholwInvView(const CholwView& v) : CholwView(v) {}
  friend AfterwView afterw_view(float* workspace, int D);
};
static_assert(sizeof(CholwInvView) == sizeof(CholwView), "both views are the same kernel argument");

// a launch does nothing for a slab that left or whose factorisation has broken down; one thread reads, all follow
__device__ __forceinline__ bool cholw_gate(const CholwCtl* ctl) {
  __shared__ int s_go;
  if (threadIdx.x == 0) s_go = ctl->active != 0 && ctl->notpd == 0;
  __syncthreads();
  return s_go != 0;
}

// log det of a factored slab = the sum of its first n log-pivots: 256 strided partial sums, combined by thread 0 in thread order (valid in
// thread 0 alone); NaN for a slab whose factorisation broke down (ok = cholw_gate's answer).  One barrier, behind the stores into s_sum.
__device__ __forceinline__ double cholw_log_pivot_sum(const CholwInvView& v, int t, int n, bool ok, double (&s_sum)[kWThreads]) {
  const double* lp = v.log_pivot(t);
  double s = 0.0;
  if (ok)
    for (int k = threadIdx.x; k < n; k += kWThreads) s += lp[k];
  s_sum[threadIdx.x] = s;
  __syncthreads();
  double sum = 0.0;
  if (threadIdx.x == 0)
    for (int k = 0; k < kWThreads; ++k) sum += s_sum[k];
  return ok ? sum : __builtin_nan("");
}

// ---------------------------------------------------------------------------------------------------------------- Cholesky, launch A
// grid (DP / 64 - j, K): tile (i, j), i = j + blockIdx.x, of L = A - sigma delta - sum_{k < 64 j} L(i, k) L(j, k)
__global__ __launch_bounds__(kWThreads) void cholw_update_kernel(int j, CholwView v) {
  __shared__ __attribute__((aligned(16))) double s_stage[2 * kT64Stage];
  const int t = blockIdx.y;
  if (!cholw_gate(v.ctl(t))) return;
  const int DP = v.DP;
  const int i0 = (j + (int)blockIdx.x) * kT64, j0 = j * kT64;
  const double* A = v.a(t);
  double* L = v.l(t);
  const double* rows[2] = {L + (size_t)i0 * DP, L + (size_t)j0 * DP};
  f64x4 acc[2][2];
  t64_zero(acc);
  t64_tile_product<true>(0, j0, [&](int which, int x, int k) { return rows[which][(size_t)x * DP + k]; }, s_stage, s_stage + kT64Stage, acc);
  const double sigma = v.ctl(t)->sigma;
  t64_for_each_fragment([&](int a, int c, int r, int row, int col) {
    const int i = i0 + row, jj = j0 + col;
    const size_t at = (size_t)i * DP + jj;
    L[at] = A[at] - (i == jj ? sigma : 0.0) - acc[a][c][r];
  });
}

// ---------------------------------------------------------------------------------------------------------------- Cholesky, launch B
// grid (DP / 64 - j, K).  Every workgroup factors the updated diagonal tile (j, j) in LDS -- thread = row (lane) x columns = wave mod 4,
// right-looking, one barrier per column; the column stays unscaled until the end so that every thread forms l_rc = a_rc / sqrt(a_cc) from the
// same bits -- and then solves its own tile X L(j, j)^T = L(i, j) column by column.  A pivot that is <= 0 or NaN ends the factorisation in
// every workgroup alike; the diagonal tile's workgroup raises the flag.  Tile (j, j) is only read here (all workgroups of the launch load it).
// View = CholwInvView: the diagonal tile's workgroup goes on to L(j, j)^-T and the log-pivots.
template <class View>
__global__ __launch_bounds__(kWThreads) void cholw_panel_kernel(int j, View v) {
  __shared__ double s_d[kT64 * kT64Ldt], s_t[kT64 * kT64Ldt], s_inv[kT64];
  const int t = blockIdx.y;
  CholwCtl* ctl = v.ctl(t);
  if (!cholw_gate(ctl)) return;
  const int tid = threadIdx.x, r = tid & 63, w = tid >> 6, DP = v.DP;
  const int i0 = (j + (int)blockIdx.x) * kT64, j0 = j * kT64;
  double* L = v.l(t);
  t64_for_each_element([&](int rr, int cc) {
    s_d[rr * kT64Ldt + cc] = L[(size_t)(j0 + rr) * DP + j0 + cc];
    s_t[rr * kT64Ldt + cc] = L[(size_t)(i0 + rr) * DP + j0 + cc];
  });
  bool bad = false;
  for (int c = 0; c < kT64; ++c) {
    __syncthreads();  // (the loads; the updates of column c - 1)
    const double d = s_d[c * kT64Ldt + c];
    if (!(d > 0.0)) {  // (also NaN; the same bits in every thread of every workgroup)
      bad = true;
      break;
    }
    const double inv = 1.0 / sqrt(d);
    if (tid == 0) s_inv[c] = inv;
    if (r > c) {
      const double lrc = s_d[r * kT64Ldt + c] * inv;
      for (int q = c + 1 + ((w - c - 1) & 3); q <= r; q += 4) s_d[r * kT64Ldt + q] -= lrc * (s_d[q * kT64Ldt + c] * inv);
    }
  }
  if (bad) {
    if (blockIdx.x == 0 && tid == 0) ctl->notpd = 1;
    return;
  }
  const bool diag = blockIdx.x == 0;
  if (diag) {
    if constexpr (!View::kKeepsInverse) return;  // (the diagonal tile's workgroup: its part was the decision)
    // the solve below on the identity instead of the tile gives L(j, j)^-T
    t64_for_each_element([&](int rr, int cc) { s_t[rr * kT64Ldt + cc] = rr == cc ? 1.0 : 0.0; });
  }
  __syncthreads();
  // X L^T = T: x_rc = (t_rc - sum_{p < c} x_rp l_cp) / l_cc, with l_qc = s_d[q][c] inv_c and l_cc = 1 / inv_c
  for (int c = 0; c < kT64; ++c) {
    const double inv = s_inv[c];
    if (w == (c & 3)) s_t[r * kT64Ldt + c] *= inv;  // (this thread owns the columns = w mod 4 of row r)
    __syncthreads();
    const double x = s_t[r * kT64Ldt + c];
    for (int q = c + 1 + ((w - c - 1) & 3); q < kT64; q += 4) s_t[r * kT64Ldt + q] -= x * (s_d[q * kT64Ldt + c] * inv);
  }
  __syncthreads();
  if constexpr (View::kKeepsInverse) {
    if (diag) {  // into the slab of the inverse, NOT over tile (j, j) of L: the other workgroups of this launch are still reading that
      double* Wt = v.inv_t(t);
      t64_for_each_element([&](int rr, int cc) { Wt[(size_t)(j0 + rr) * DP + j0 + cc] = cc >= rr ? s_t[rr * kT64Ldt + cc] : 0.0; });
      if (tid < kT64) v.log_pivot(t)[j0 + tid] = log(s_d[tid * kT64Ldt + tid]);
      return;
    }
  }
  t64_for_each_element([&](int rr, int cc) { L[(size_t)(i0 + rr) * DP + j0 + cc] = s_t[rr * kT64Ldt + cc]; });
}

// ---------------------------------------------------------------------------------------------------------------- the shift bisection
constexpr double kCholwThreshold = 1e-6;  // prepare_data.py:347

// grid (K), one wave, between two factorisations: reads the "not PD" flag, moves the bracket, chooses the next sigma.  step -1: before the
// first factorisation (sigma = the threshold); step 0: its result -- positive definite there: no repair, the slab leaves; else the bracket
// [Bracket::lower, threshold]; steps 1 .. Bracket::kSteps: positive definite => lo = sigma, else hi = sigma.
// Bracket (the client's): static constexpr int kSteps; __device__ static double lower(const CholwView&, int t, int D), called by the whole
// wave, every sum in it in a fixed order.
template <class Bracket>
__global__ __launch_bounds__(64) void cholw_bisect_kernel(int step, int D, CholwView v) {
  const int t = blockIdx.x, lane = threadIdx.x;
  CholwCtl* ctl = v.ctl(t);
  double lower = 0.0;
  if (step == 0) lower = Bracket::lower(v, t, D);
  if (lane != 0) return;
  if (step < 0) {
    ctl->reset(kCholwThreshold);
    return;
  }
  if (!ctl->active) return;
  const bool pd = ctl->notpd == 0;
  if (step == 0) {
    if (pd) {
      ctl->active = 0;
      return;
    }
    ctl->lo = lower;
    ctl->hi = kCholwThreshold;
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

// The bisection's last step.  grid (ceil(D / 256), K): A += (eval_offset - min eig) I for the slabs that failed the test at the threshold, the
// diagonal of the fp32 output rewritten from it (one rounding); min_eig_out[t] = the smallest eigenvalue before the repair, or +infinity for
// a slab that passed (its eigenvalue is never computed)
__global__ __launch_bounds__(256) void cholw_repair_kernel(int D, double eval_offset, CholwView v, float* __restrict__ A_out,
                                                           double* __restrict__ min_eig_out) {
  const int t = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  CholwCtl* ctl = v.ctl(t);
  const bool active = ctl->active != 0;
  const double mn = ctl->min_eig;
  if (active && i < D) {
    double* A = v.a(t);
    const double d = A[(size_t)i * v.DP + i] + (eval_offset - mn);
    A[(size_t)i * v.DP + i] = d;
    A_out[(size_t)t * D * D + (size_t)i * D + i] = (float)d;
  }
  if (i == 0) {
    min_eig_out[t] = active ? mn : __builtin_inf();
    ctl->repaired = active ? 1 : 0;
  }
}

}  // namespace uglad
