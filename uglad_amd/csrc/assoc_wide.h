// The association matrix of a table that mixes categorical and real columns (uglad_association; the reference's pairwise_cov_matrix,
// prepare_data.py:177-285: bias-corrected Cramer's V for c/c pairs, the correlation ratio eta for c/r pairs, Pearson's r for r/r pairs),
// fp64 throughout, on the tile layer of chol_wide.h, and the reference's repair (prepare_data.py:347-352) for a matrix that is NOT a Gram
// matrix.
//
// The table arrives encoded (N x D fp64: a categorical column holds level codes 0 .. card - 1, a real column its values) with the maps of
// its EXPANDED layout: W columns, one per level of every categorical (0 / 1) and one per real column (centred, scaled to unit norm).  The
// expanded table E is never stored -- the tile product's loader makes its elements -- and the one Gram product E^T E holds every
// contingency table (c/c blocks, exact integers), every per-level sum of every unit-norm real column (c/r blocks) and every Pearson
// coefficient (r/r entries).  The host lays the expanded columns out so that a feature's columns never straddle a multiple of 64: the
// block of a pair of features then lies inside exactly ONE 64 x 64 Gram tile, and the workgroup that formed the tile finishes its pairs.
//
//   assoc_stats_kernel    per table and block of 64 expanded columns: mean and 1 / sqrt(sum (x - mean)^2) of a real column, the count
//                         n_a of a level column (rows over waves, combined in wave order); also writes the identity into the slab's padding
//   assoc_gram_kernel     one workgroup per upper tile pair (I <= J) of the expanded width: the Gram tile on the fp64 MFMA, through
//                         t64_for_each_fragment into LDS; then thread p takes the p-th pair of features (i <= j) whose block lies in this
//                         tile and writes ONE entry of the D x D result into both triangles (the mirror is a copy) of the fp64 slab
//                         (CholwView::a, row stride DP), the optional fp64 output and the fp32 output
//   assoc_rowsum_kernel   sum_r |A(r, i)| per column i (= row: A is symmetric to the bit) -> vec3
//   the shift bisection of chol_wide.h on AssocBracket (launch_cholw_bisection, as in cov_wide.h): the bracket of an INDEFINITE symmetric
//                         matrix, [-||A||_inf, 1e-6] (every eigenvalue lies in [-||A||_inf, ||A||_inf]; V and eta are >= 0 while r is
//                         signed, so A is far from positive semi-definite and cov_wide.h's -2^-30 tr S would not bracket), 48 steps: the
//                         bracket ends at ||A||_inf 2^-48
//
// A thread, not a wave, takes a pair: at the usual cardinalities (2 .. 12) a tile holds hundreds of pairs of a few dozen cells each, and a
// serial sum per pair has one fixed order.  Every sum has a fixed order; nothing reads back to the host.
#pragma once
#include "cov_wide.h"

namespace uglad {

constexpr int kAssocReal = -1;       // col_level of a real feature's column
constexpr int kAssocPad = -2;        // col_level of a padding column (col_feature -1)
constexpr int kAssocMaxWidth = 16384;  // W: 256 x 256 tile pairs per table

// the expanded layout, DEVICE pointers (made by uglad_amd.utils.prepare_data.encode_mixed_table)
struct AssocMaps {
  const int* col_feature;  // [W]  feature of an expanded column, -1: padding
  const int* col_level;    // [W]  level >= 0 | kAssocReal | kAssocPad
  const int* feat_offset;  // [D]  first expanded column of a feature
  const int* feat_width;   // [D]  its number of expanded columns (all inside one tile of 64)
  const int* tile_first;   // [W / 64 + 1]  first feature of a tile of 64 expanded columns; the last entry is D
  int W;                   // a multiple of 64
};

// A table's part of the workspace, in DOUBLES: the factorisation's slab (chol_wide.h; A = the association matrix, vec3[0 .. D) = its
// absolute row sums) and behind it the column statistics  mean[W] | scale-or-count[W].
__host__ __device__ constexpr size_t assoc_table_doubles(int DP, int W) { return cholw_slab_doubles(DP) + 2 * (size_t)W; }
__host__ inline CholwView assoc_view(float* workspace, int D, int W) {
  const int DP = t64_padded(D);
  return CholwView{reinterpret_cast<double*>(workspace), assoc_table_doubles(DP, W), DP};
}
__host__ __device__ inline double* assoc_stats(const CholwView& v, int t) { return v.a(t) + cholw_slab_doubles(v.DP); }

// ---------------------------------------------------------------------------------------------------------------- column statistics
// grid (W / 64, K): thread = expanded column (lane) x row group (wave); rows w, w + 4, ...; the four partial results combined in wave order
__global__ __launch_bounds__(kWThreads) void assoc_stats_kernel(const double* __restrict__ X, int N, int D, AssocMaps m, CholwView v) {
  __shared__ double s_p[4][kT64];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, t = blockIdx.y;
  const int c = blockIdx.x * kT64 + lane;
  const int f = m.col_feature[c], lv = m.col_level[c];
  const bool live = f >= 0 && f < D && lv >= kAssocReal;
  const double* Xc = X + (size_t)t * N * D + (live ? f : 0);
  double part = 0.0;  // a level column: its count; a real column: its sum
  if (live)
    for (int n = w; n < N; n += 4) {
      const double x = Xc[(size_t)n * D];
      part += lv >= 0 ? (x == (double)lv ? 1.0 : 0.0) : x;
    }
  const double total = t64_sum_waves(part, s_p);
  const double mean = total / (double)N;
  __syncthreads();  // (s_p is used again)
  double ss = 0.0;
  if (live && lv == kAssocReal)
    for (int n = w; n < N; n += 4) {
      const double d = Xc[(size_t)n * D] - mean;
      ss += d * d;
    }
  ss = t64_sum_waves(ss, s_p);
  if (w == 0) {
    double* st = assoc_stats(v, t);
    const bool real = live && lv == kAssocReal;
    st[c] = real ? mean : 0.0;
    st[m.W + c] = real ? 1.0 / sqrt(ss) : (live ? total : 0.0);  // (a constant real column: 1 / 0, NaN in its row and column)
  }
  // the slab's padding carries the identity: the strip of columns D .. DP and its mirror, the launch's threads striding it
  const int DP = v.DP, pad = DP - D;
  double* S64 = v.a(t);
  for (int idx = blockIdx.x * kWThreads + tid; idx < DP * pad; idx += gridDim.x * kWThreads) {
    const int i = idx / pad, j = D + idx % pad;
    S64[(size_t)i * DP + j] = S64[(size_t)j * DP + i] = i == j ? 1.0 : 0.0;
  }
}

// ---------------------------------------------------------------------------------------------------------------- one pair of features
// tile[x * kT64Ldt + y] = sum_n E(n, I 64 + x) E(n, J 64 + y); feature i owns rows oi .. oi + wi of it, feature j columns oj .. oj + wj;
// cnt_i / cnt_j: the level counts of the tile's rows / columns; n = N
__device__ inline double assoc_pair(const double* tile, const double* cnt_i, const double* cnt_j, int oi, int wi, bool cat_i, int oj,
                                    int wj, bool cat_j, double n) {
  if (!cat_i && !cat_j) return tile[oi * kT64Ldt + oj];  // Pearson's r
  if (cat_i != cat_j) {  // eta = sqrt(sum_a s_a^2 / n_a) over the levels that occur; exactly 0 stays 0 (the reference's numerator == 0)
    const int wc = cat_i ? wi : wj;
    double sum = 0.0;
    for (int a = 0; a < wc; ++a) {
      const double na = cat_i ? cnt_i[oi + a] : cnt_j[oj + a];
      const double s = cat_i ? tile[(oi + a) * kT64Ldt + oj] : tile[oi * kT64Ldt + oj + a];
      if (na > 0.0) sum += s * s / na;
    }
    return sum == 0.0 ? 0.0 : sqrt(sum);
  }
  // Cramer's V, bias-corrected (prepare_data.py:196-209), of the contingency table without its empty rows and columns (pd.crosstab)
  int r = 0, k = 0;
  for (int a = 0; a < wi; ++a) r += cnt_i[oi + a] > 0.0;
  for (int b = 0; b < wj; ++b) k += cnt_j[oj + b] > 0.0;
  const bool yates = (r - 1) * (k - 1) == 1;  // chi2_contingency: one degree of freedom
  double chi2 = 0.0;
  for (int a = 0; a < wi; ++a) {
    const double na = cnt_i[oi + a];
    if (!(na > 0.0)) continue;
    for (int b = 0; b < wj; ++b) {
      const double nb = cnt_j[oj + b];
      if (!(nb > 0.0)) continue;
      const double E = na * nb / n;
      double O = tile[(oi + a) * kT64Ldt + oj + b];
      if (yates) {  // every observed count moves towards its expected count by min(1/2, |O - E|)
        const double diff = E - O, mag = fmin(0.5, fabs(diff));
        O += diff > 0.0 ? mag : (diff < 0.0 ? -mag : 0.0);
      }
      const double d = O - E;
      chi2 += d * d / E;
    }
  }
  const double rr = (double)r, kk = (double)k;
  const double phi2corr = fmax(0.0, chi2 / n - (kk - 1.0) * (rr - 1.0) / (n - 1.0));
  const double rcorr = rr - (rr - 1.0) * (rr - 1.0) / (n - 1.0), kcorr = kk - (kk - 1.0) * (kk - 1.0) / (n - 1.0);
  const double denom = fmin(kcorr - 1.0, rcorr - 1.0);
  return denom == 0.0 ? 0.0 : sqrt(phi2corr / denom);
}

// ---------------------------------------------------------------------------------------------------------------- Gram + pair reduction
// grid (W / 64, W / 64, K); tile pairs below the diagonal return.  Rows >= N and padding columns are zero.
__global__ __launch_bounds__(kWThreads) void assoc_gram_kernel(const double* __restrict__ X, int N, int D, AssocMaps m, CholwView v,
                                                               double* __restrict__ A64_out, float* __restrict__ A_out) {
  __shared__ __attribute__((aligned(16))) double s_stage[2 * kT64Stage];
  __shared__ double s_cnt[2][kT64];
  static_assert(kT64 * kT64Ldt <= 2 * kT64Stage, "the whole tile fits the staging area it takes over");
  const int I = blockIdx.y, J = blockIdx.x, t = blockIdx.z;
  if (I > J) return;  // (uniform per workgroup)
  const int tid = threadIdx.x, lane = tid & 63, DP = v.DP, W = m.W;
  const double* Xt = X + (size_t)t * N * D;
  const double* st = assoc_stats(v, t);
  // a thread stages the same expanded column of either operand in every chunk (256 = 0 mod 64)
  const int col[2] = {I * kT64 + lane, J * kT64 + lane};
  int f[2], lv[2];
  double mu[2], sc[2];
  for (int q = 0; q < 2; ++q) {
    f[q] = m.col_feature[col[q]], lv[q] = m.col_level[col[q]];
    if (f[q] < 0 || f[q] >= D || lv[q] < kAssocReal) lv[q] = kAssocPad, f[q] = 0;
    mu[q] = st[col[q]], sc[q] = st[W + col[q]];
  }
  if (tid < kT64) s_cnt[0][lane] = lv[0] >= 0 ? sc[0] : 0.0, s_cnt[1][lane] = lv[1] >= 0 ? sc[1] : 0.0;
  f64x4 acc[2][2];
  t64_zero(acc);
  t64_tile_product<false>(0, N, [&](int which, int, int n) {
    if (n >= N || lv[which] == kAssocPad) return 0.0;
    const double x = Xt[(size_t)n * D + f[which]];
    return lv[which] >= 0 ? (x == (double)lv[which] ? 1.0 : 0.0) : (x - mu[which]) * sc[which];
  }, s_stage, s_stage + kT64Stage, acc);
  __syncthreads();  // (the last chunk has been consumed: the staging area becomes the tile)
  double* s_tile = s_stage;
  t64_for_each_fragment([&](int a, int c, int r, int row, int cl) { s_tile[row * kT64Ldt + cl] = acc[a][c][r]; });
  __syncthreads();
  const int fi0 = m.tile_first[I], ni = m.tile_first[I + 1] - fi0, fj0 = m.tile_first[J], nj = m.tile_first[J + 1] - fj0;
  double* S64 = v.a(t);
  for (int p = tid; p < ni * nj; p += kWThreads) {
    const int i = fi0 + p / nj, j = fj0 + p % nj;
    if (i > j || i < 0 || j >= D) continue;  // (i > j: the diagonal tile pair; its lower half is the mirror of its upper half)
    const int oi = m.feat_offset[i] - I * kT64, wi = m.feat_width[i], oj = m.feat_offset[j] - J * kT64, wj = m.feat_width[j];
    if (oi < 0 || wi < 1 || oi + wi > kT64 || oj < 0 || wj < 1 || oj + wj > kT64) continue;  // (a layout that breaks the rule)
    const bool cat_i = m.col_level[I * kT64 + oi] >= 0, cat_j = m.col_level[J * kT64 + oj] >= 0;
    const double val = assoc_pair(s_tile, s_cnt[0], s_cnt[1], oi, wi, cat_i, oj, wj, cat_j, (double)N);
    S64[(size_t)i * DP + j] = val;
    S64[(size_t)j * DP + i] = val;
    if (A64_out) {
      double* Ao = A64_out + (size_t)t * D * D;
      Ao[(size_t)i * D + j] = val;
      Ao[(size_t)j * D + i] = val;
    }
    float* Af = A_out + (size_t)t * D * D;
    Af[(size_t)i * D + j] = (float)val;
    Af[(size_t)j * D + i] = (float)val;
  }
}

// ---------------------------------------------------------------------------------------------------------------- ||A||_inf, row by row
// grid (ceil(D / 256), K): thread i sums |A(r, i)| down column i (A is symmetric to the bit; the threads of a wave read one row together)
__global__ __launch_bounds__(256) void assoc_rowsum_kernel(int D, CholwView v) {
  const int t = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  if (i >= D) return;
  const double* S64 = v.a(t);
  double s = 0.0;
  for (int r = 0; r < D; ++r) s += fabs(S64[(size_t)r * v.DP + i]);
  v.vec3(t)[i] = s;
}

// the bisection's bracket: lower end -||A||_inf = -max of the row sums (a maximum: any order gives the same bits)
struct AssocBracket {
  static constexpr int kSteps = 48;  // bisection steps behind the test at the threshold
  __device__ static double lower(const CholwView& v, int t, int D) {
    const double* rs = v.vec3(t);
    double nrm = 0.0;
    for (int i = (int)threadIdx.x; i < D; i += 64) nrm = fmax(nrm, rs[i]);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) nrm = fmax(nrm, __shfl_xor(nrm, off));
    return -nrm;
  }
};

}  // namespace uglad
