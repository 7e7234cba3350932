// The rank-based correlation matrix of a table (uglad_rank_correlation): the front-end of the nonparanormal (Gaussian copula) model, which
// replaces the covariance of a table by Spearman's rho mapped through 2 sin(pi rho / 6), Kendall's tau-b mapped through sin(pi tau / 2)
// (Liu, Han, Yuan, Lafferty, Wasserman 2012) or the correlation of the normal scores Phi^-1(rank / (N + 1)); fp64 and exact integers
// throughout, on the slab, the Gram product, the bracket and the repair of chol_wide.h, cov_wide.h and assoc_wide.h.
//
//   rank_kernel           per table, column and block of 256 rows: the DOUBLED midrank r2_a = 2 #{b : x_b < x_a} + #{b : x_b = x_a} + 1 of
//                         every row (an int32, twice scipy's rankdata(method="average")) by counting against the column, which passes
//                         through LDS 256 values at a time; the column's flags (bit 0: holds a NaN, bit 1: constant).  Kendall: r2 goes
//                         column-major into the ranks block; Spearman: c = r2 - (N + 1) (the doubled midranks of a column have mean N + 1
//                         exactly) and scores: z = Phi^-1(r2 / (2 (N + 1))) go into a (K, N, D) fp64 table
//   Spearman, scores      covw_stats_kernel + covw_gram_kernel<RankGramSink> on that table: the centred sums sum_a c_ai c_aj.  For Spearman
//                         every column sum is exactly 0 and every product and partial sum an integer below 2^48: exact in any order
//   rank_kendall_kernel   Kendall: with s[(a, b), i] = sign(r2_ai - r2_bi) over the P = N (N - 1) / 2 row pairs a < b, G = s^T s has
//                         G_ij = concordant - discordant pairs and G_ii = P - (pairs tied in column i), and tau-b is exactly
//                         G_ij / (sqrt(G_ii) sqrt(G_jj)): tau is the "correlation" of an integer Gram matrix.  One workgroup per upper
//                         T x T tile of G and chunk of pairs, on v_mfma_i32_16x16x64_i8; the signs are made on the fly from the ranks, once
//                         per workgroup, and shared through LDS as packed int8; the int32 partial tiles are combined by integer atomics
//                         (exact, so any order gives the same bits)
//   rank_finish_kernel    rho_ij = g_ij / (sqrt(g_ii) sqrt(g_jj)) (two square roots: G_ii G_jj passes 2^53), the transform, exactly 1 on the
//                         diagonal, NaN in the row and column of a flagged feature; both triangles (the mirror is a copy) of the slab, of
//                         the fp32 output and of the optional fp64 outputs
//   assoc_rowsum_kernel, launch_cholw_bisection<AssocBracket>: the transforms do not preserve positive semi-definiteness, so the repair
//                         is uglad_association's, the 48-step bracket of an indefinite matrix
//
// The pairs are enumerated by shift: for t = 1 .. N - 1 the pairs (a, a + t), a = 0 .. N - t - 1, are contiguous in a, so a step of 64 pairs
// reads two runs of 64 ranks per feature and needs no triangular mask; the tail of a shift is padded with zero signs, which add nothing.
// Pair chunk c of n takes the shifts c + 1, c + 1 + n, ...: interleaved, every chunk gets long and short shifts alike.
// Nothing reads back to the host; nothing is allocated.
#pragma once
#include "assoc_wide.h"

namespace uglad {

constexpr int kRankSpearman = 0, kRankKendall = 1, kRankScores = 2;
constexpr int kRankMaxN = 65536;     // G_ii <= N (N - 1) / 2 < 2^31
constexpr int kRankStep = 64;        // pairs per MFMA step (the k of v_mfma_i32_16x16x64_i8)
constexpr int kRankLd = 80;          // LDS row stride, in bytes, of a [feature][64 signs] operand (16-byte aligned, 20 banks)
constexpr int kRankTileNarrow = 64;  // T for D <= 128, else 128
constexpr int kRankTileWide = 128;
typedef int i32x4 __attribute__((ext_vector_type(4)));

// acc += A B on v_mfma_i32_16x16x64_i8: lane l gives 16 consecutive k, k = 16 (l >> 4) + j, of A's row / B's column l & 15 as the 16 bytes
// of its four registers (byte j & 3 of register j >> 2); C register r of lane l is C[4 (l >> 4) + r][l & 15].
#ifndef UGLAD_SIMT_EMUL
__device__ __forceinline__ i32x4 rank_mfma_i8(i32x4 a, i32x4 b, i32x4 c) { return __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, c, 0, 0, 0); }
#else
// The host build (as UGLAD_WAVE_SYNC in glad_device.h: the emulator's runtime header has no such instruction): the same lane conventions
// on the emulator's wave-wide operand exchange, the two operands in two rounds through its 64-bit slots.
inline i32x4 rank_mfma_i8(i32x4 a, i32x4 b, i32x4 c) {
  simt::State& s = simt::st();
  simt::WaveState& w = simt::my_wave();
  simt::Fiber& f = s.fibers[s.cur];
  const int lane = s.cur % simt::kWave, col = lane & 15;
  signed char ak[4][64], bk[64];  // this lane's four rows of A and its column of B, k = 0 .. 63
  for (int round = 0; round < 2; ++round) {
    const int par = f.n_coll++ & 1;
    const i32x4 mine = round ? b : a;
    memcpy(&w.slot64a[par][lane], &mine, 8);
    memcpy(&w.slot64b[par][lane], reinterpret_cast<const char*>(&mine) + 8, 8);
    simt::wave_sync();
    for (int kq = 0; kq < 4; ++kq) {
      if (round) {
        memcpy(bk + 16 * kq, &w.slot64a[par][16 * kq + col], 8);
        memcpy(bk + 16 * kq + 8, &w.slot64b[par][16 * kq + col], 8);
      } else {
        for (int r = 0; r < 4; ++r) {
          memcpy(ak[r] + 16 * kq, &w.slot64a[par][16 * kq + 4 * (lane >> 4) + r], 8);
          memcpy(ak[r] + 16 * kq + 8, &w.slot64b[par][16 * kq + 4 * (lane >> 4) + r], 8);
        }
      }
    }
  }
  for (int r = 0; r < 4; ++r) {
    int acc = c[r];
    for (int k = 0; k < 64; ++k) acc += (int)ak[r][k] * (int)bk[k];
    c[r] = acc;
  }
  return c;
}
#endif

__host__ __device__ constexpr int rank_tile(int D) { return D > 2 * kRankTileNarrow ? kRankTileWide : kRankTileNarrow; }
__host__ __device__ constexpr int rank_padded_rows(int N) { return (N + 63) / 64 * 64 + 64; }  // a step reads up to row N + 62
__host__ __device__ constexpr int rank_padded_tiles(int D) { return (D + rank_tile(D) - 1) / rank_tile(D) * rank_tile(D); }

// The workspace, in DOUBLES: K slabs of chol_wide.h, each followed by the DP column flags (int32); behind them, at the next multiple of 16
// bytes (the Kendall kernel reads four ranks at a time), one block for all tables:
//   Kendall            ranks  K x D x NP int32 (column-major per table, NP = rank_padded_rows(N)) | G  K x DT x DT int32 (DT = D rounded up to T)
//   Spearman, scores   the (K, N, D) fp64 table of c or z
struct RankView {
  CholwView c;
  double* block;  // behind the K slabs
  int K, NP, DT;
  __host__ __device__ int* info(int t) const { return reinterpret_cast<int*>(c.a(t) + cholw_slab_doubles(c.DP)); }
  __host__ __device__ int* ranks(int t, int D) const { return reinterpret_cast<int*>(block) + (size_t)t * D * NP; }
  __host__ __device__ int* gram32(int t, int D) const { return reinterpret_cast<int*>(block) + (size_t)K * D * NP + (size_t)t * DT * DT; }
  __host__ __device__ double* table() const { return block; }
};
__host__ __device__ constexpr size_t rank_slab_doubles(int DP) { return cholw_slab_doubles(DP) + (size_t)DP / 2; }
__host__ inline size_t rank_table_floats(int N, int D, int method) {
  const size_t DT = rank_padded_tiles(D);
  const size_t block = method == kRankKendall ? (size_t)D * rank_padded_rows(N) + DT * DT : 2 * (size_t)N * D;  // (both even)
  return 2 * rank_slab_doubles(t64_padded(D)) + block + 2;  // (+ 2: the block starts at a multiple of 16 bytes, the workspace at one of 8)
}
__host__ inline RankView rank_view(float* workspace, int K, int N, int D) {
  const int DP = t64_padded(D);
  double* base = reinterpret_cast<double*>(workspace);
  const size_t block = (reinterpret_cast<size_t>(base + (size_t)K * rank_slab_doubles(DP)) + 15) & ~(size_t)15;  // (the 2 spare floats)
  return RankView{CholwView{base, rank_slab_doubles(DP), DP}, reinterpret_cast<double*>(block), K, rank_padded_rows(N), rank_padded_tiles(D)};
}

// ---------------------------------------------------------------------------------------------------------------- Phi^-1
// Phi^-1(num / den) for 0 < num < den, plain fp64 (the same routine in every build): Acklam's rational approximation (relative error
// 1.2e-9) at p = min(num, den - num) / den <= 1/2, then two Halley steps on Phi(x) - p with erfc -- cubic convergence, so what is left is
// erfc's own rounding: |error| <~ 2^-52 max(|x|, 1/2).  The upper half is the mirror image, taken on the integers: exactly odd about 1/2.
__host__ __device__ inline double rank_ndtri(int num, int den) {
  const int low = num < den - num ? num : den - num;
  const double p = (double)low / (double)den;
  double x;
  if (p < 0.02425) {
    const double q = sqrt(-2.0 * log(p));
    x = (((((-7.784894002430293e-03 * q - 3.223964580411365e-01) * q - 2.400758277161838e+00) * q - 2.549732539343734e+00) * q +
          4.374664141464968e+00) * q + 2.938163982698783e+00) /
        ((((7.784695709041462e-03 * q + 3.224671290700398e-01) * q + 2.445134137142996e+00) * q + 3.754408661907416e+00) * q + 1.0);
  } else {
    const double q = p - 0.5, r = q * q;
    x = (((((-3.969683028665376e+01 * r + 2.209460984245205e+02) * r - 2.759285104469687e+02) * r + 1.383577518672690e+02) * r -
          3.066479806614716e+01) * r + 2.506628277459239e+00) * q /
        (((((-5.447609879822406e+01 * r + 1.615858368580409e+02) * r - 1.556989798598866e+02) * r + 6.680131188771972e+01) * r -
          1.328068155288572e+01) * r + 1.0);
  }
  for (int it = 0; it < 2; ++it) {
    const double e = 0.5 * erfc(-x * 0.70710678118654752440) - p;
    const double u = e * 2.50662827463100050242 * exp(0.5 * x * x);  // e / phi(x)
    x -= u / (1.0 + 0.5 * x * u);
  }
  return num == low ? x : -x;
}

// ---------------------------------------------------------------------------------------------------------------- ranks
// grid (ceil(N / 256), D, K): thread = row a of column i; the column passes through LDS 256 rows at a time, every thread counting the
// staged values below and equal to its own (a NaN counts as neither).  Every thread sees the whole column, so thread 0 of block 0 knows
// the flags.
__global__ __launch_bounds__(kWThreads) void rank_kernel(const double* __restrict__ X, int N, int D, int method, RankView v,
                                                         int* __restrict__ info_out) {
  __shared__ double s_x[kWThreads];
  const int tid = threadIdx.x, i = blockIdx.y, t = blockIdx.z, a = blockIdx.x * kWThreads + tid;
  const double* Xc = X + (size_t)t * N * D + i;
  const double x = a < N ? Xc[(size_t)a * D] : 0.0;
  int lt = 0, eq = 0;
  bool nan = false;
  for (int b0 = 0; b0 < N; b0 += kWThreads) {
    __syncthreads();  // (the previous chunk has been consumed)
    if (b0 + tid < N) s_x[tid] = Xc[(size_t)(b0 + tid) * D];
    __syncthreads();
    const int nb = N - b0 < kWThreads ? N - b0 : kWThreads;
    for (int q = 0; q < nb; ++q) {
      const double y = s_x[q];
      lt += y < x ? 1 : 0;
      eq += y == x ? 1 : 0;
      nan = nan || y != y;
    }
  }
  if (a == 0) {
    const int flags = nan ? 1 : (eq == N ? 2 : 0);
    v.info(t)[i] = flags;
    if (info_out) info_out[(size_t)t * D + i] = flags;
  }
  if (a >= N) return;
  const int r2 = 2 * lt + eq + 1;  // 1 (a NaN) .. 2 N
  if (method == kRankKendall) v.ranks(t, D)[(size_t)i * v.NP + a] = r2;
  else v.table()[((size_t)t * N + a) * D + i] = method == kRankSpearman ? (double)(r2 - (N + 1)) : rank_ndtri(r2, 2 * (N + 1));
}

// covw_gram_kernel's sink for the table of c or z: the centred SUMS (not / N: Spearman's are exact integers), upper triangle, into the
// slab's second matrix, which nothing else uses before the factorisation
struct RankGramSink {
  using View = CholwView;
  using Out = double;
  static constexpr bool kSums = true;
  CholwView v;
  double* unused;
  int D;
  __device__ void put(int t, int i, int j, double sum, bool inside) const {
    if (inside) v.l(t)[(size_t)i * v.DP + j] = sum;
  }
  __device__ void finish(int, int, int) const {}
};

// ---------------------------------------------------------------------------------------------------------------- Kendall's Gram matrix
// grid (nt (nt + 1) / 2, chunks, K), nt = DT / T, T = 32 TB: upper tile (I, J) of G over the shifts blockIdx.y + 1, + gridDim.y, ...
// Wave w owns rows 16 TB (w >> 1) .., columns 16 TB (w & 1) .. of the tile as TB x TB accumulators; acc[a][c][r] of lane l is
// C[16 a + 4 (l >> 4) + r][16 c + (l & 15)] (the C/D map of every 16 x 16 MFMA but the fp64 one).  Operands: lane l holds 16 consecutive k,
// k = 16 (l >> 4) + j, of row (A) / column (B) l & 15; both operands are made by the same rule and the sum over k is order-free, so any k
// assignment they share is right.  A step: thread -> (feature row, 4 pairs) of either operand -- sixteen lanes read 64 consecutive ranks of a
// row, 256 contiguous bytes, and the same run `shift` rows on -- and packs its 4 signs into one LDS word; two LDS buffers in turn, so one barrier per step.  The diagonal tile makes one operand and reads it twice.
template <int TB>
__global__ __launch_bounds__(kWThreads) void rank_kendall_kernel(int N, int D, RankView v) {
  constexpr int T = 32 * TB, kUnits = T * 16 / kWThreads;
  __shared__ __attribute__((aligned(16))) signed char s_sign[2][2][T * kRankLd];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, t = blockIdx.z;
  const int l16 = lane & 15, kq = lane >> 4, ri = (w >> 1) * 16 * TB, rj = (w & 1) * 16 * TB;
  const int nt = v.DT / T;
  int I = 0, J = blockIdx.x;
  while (J >= nt - I) J -= nt - I, ++I;
  J += I;
  const bool diag = I == J;
  const int NP = v.NP;
  const int* R = v.ranks(t, D);
  i32x4 acc[TB][TB];
#pragma unroll
  for (int a = 0; a < TB; ++a)
#pragma unroll
    for (int c = 0; c < TB; ++c) acc[a][c] = (i32x4){0, 0, 0, 0};
  int buf = 0;
  for (int shift = 1 + (int)blockIdx.y; shift < N; shift += (int)gridDim.y) {
    const int np = N - shift;  // pairs (a, a + shift), a < np
    for (int a0 = 0; a0 < np; a0 += kRankStep) {
#pragma unroll
      for (int g = 0; g < kUnits; ++g) {
        const int idx = tid + kWThreads * g, row = idx >> 4, k0 = 4 * (idx & 15);
        const int left = np - (a0 + k0);  // pairs of this run of 4 that exist
#pragma unroll
        for (int which = 0; which < 2; ++which) {
          if (which && diag) continue;
          const int f = (which ? J : I) * T + row;
          unsigned word = 0;
          if (f < D && left > 0) {
            const int* ra = R + (size_t)f * NP + a0 + k0;  // (16-byte aligned: R is, and NP, a0, k0 are multiples of 4)
            const int* rb = ra + shift;  // (reads up to row a0 + 63 + shift <= N + 62 < NP; what lies beyond N is masked)
            const i32x4 va = *reinterpret_cast<const i32x4*>(ra);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const int d = (int)((unsigned)va[j] - (unsigned)rb[j]);  // (unsigned: the masked padding may hold anything)
              const int sg = j < left ? (d > 0 ? 1 : (d < 0 ? -1 : 0)) : 0;
              word |= (unsigned)(sg & 0xff) << (8 * j);
            }
          }
          *reinterpret_cast<unsigned*>(&s_sign[buf][which][row * kRankLd + k0]) = word;
        }
      }
      __syncthreads();  // (also: every wave is done with the other buffer's previous step)
      const signed char* sa = s_sign[buf][0];
      const signed char* sb = diag ? sa : s_sign[buf][1];
      i32x4 af[TB], bf[TB];
#pragma unroll
      for (int a = 0; a < TB; ++a) af[a] = *reinterpret_cast<const i32x4*>(sa + (ri + 16 * a + l16) * kRankLd + 16 * kq);
#pragma unroll
      for (int c = 0; c < TB; ++c) bf[c] = *reinterpret_cast<const i32x4*>(sb + (rj + 16 * c + l16) * kRankLd + 16 * kq);
#pragma unroll
      for (int a = 0; a < TB; ++a)
#pragma unroll
        for (int c = 0; c < TB; ++c) acc[a][c] = rank_mfma_i8(af[a], bf[c], acc[a][c]);
      buf ^= 1;
    }
  }
  int* G = v.gram32(t, D);
#pragma unroll
  for (int a = 0; a < TB; ++a)
#pragma unroll
    for (int c = 0; c < TB; ++c)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = I * T + ri + 16 * a + 4 * kq + r, j = J * T + rj + 16 * c + l16;  // (< DT)
        if (i <= j && j < D && acc[a][c][r] != 0) atomicAdd(G + (size_t)i * v.DT + j, acc[a][c][r]);
      }
}

// ---------------------------------------------------------------------------------------------------------------- the matrix
// grid (DP DP / 256, K): thread = element (i, j) of the padded matrix, i <= j; the identity in the slab's padding
__global__ __launch_bounds__(kWThreads) void rank_finish_kernel(int D, int method, int transform, RankView v, float* __restrict__ A_out,
                                                                double* __restrict__ A64_out, double* __restrict__ gram_out) {
  const int t = blockIdx.y, DP = v.c.DP;
  const int idx = blockIdx.x * kWThreads + threadIdx.x, i = idx / DP, j = idx % DP;
  if (i > j) return;
  double* S64 = v.c.a(t);
  if (j >= D) {
    covw_store(S64, DP, i, j, i == j ? 1.0 : 0.0, i != j);
    return;
  }
  double g, gi, gj;
  if (method == kRankKendall) {
    const int* G = v.gram32(t, D);
    g = (double)G[(size_t)i * v.DT + j], gi = (double)G[(size_t)i * v.DT + i], gj = (double)G[(size_t)j * v.DT + j];
  } else {
    const double* G = v.c.l(t);
    g = G[(size_t)i * DP + j], gi = G[(size_t)i * DP + i], gj = G[(size_t)j * DP + j];
  }
  const int flags = v.info(t)[i] | v.info(t)[j];
  double val = __builtin_nan("");
  if (!flags) {
    val = g / (sqrt(gi) * sqrt(gj));
    if (transform && method == kRankSpearman) val = 2.0 * sin(3.14159265358979323846 * val / 6.0);
    if (transform && method == kRankKendall) val = sin(3.14159265358979323846 * val / 2.0);
    if (i == j) val = 1.0;
  }
  const size_t off = (size_t)t * D * D;
  covw_store(S64, DP, i, j, val, i != j);
  covw_store(A_out + off, D, i, j, (float)val, i != j);
  if (A64_out) covw_store(A64_out + off, D, i, j, val, i != j);
  if (gram_out) covw_store(gram_out + off, D, i, j, (flags & 1) ? __builtin_nan("") : g, i != j);
}

}  // namespace uglad
