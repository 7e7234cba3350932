// The reference's ranking of highly correlated features (get_highly_correlated_features, prepare_data.py:519-550) on the device, fp64, for
// K covariance matrices of 2 <= D <= the cell's own limit (uglad_correlated_features): cov2 = the covariance of the matrix's rows with a zero
// diagonal; th = the element at index floor(0.1 n) of the n = D (D - 1) / 2 upper-triangle magnitudes in DESCENDING order; a feature's count =
// the entries of its row of |cov2| that are >= th (the zero diagonal included: it counts when th = 0); features by count descending, ties by
// index ascending, which is the reference's dict insertion order under its stable sort.
//
//   covw_stats_kernel, covw_gram_kernel<EigwGramSink>
//                                         cov2 into the slab of eigvals_wide.h's layout: cov_wide.h's centred Gram product with the D x D
//                                         matrix as the table (N = D)
//   corrw_init_kernel                     the rank wanted, an empty prefix, empty bins
//   8 x { corrw_hist_kernel, corrw_narrow_kernel }
//                                         a most-significant-digit-first radix SELECT on the 64-bit pattern of |x| (which orders non-negative
//                                         doubles), 8 bits per pass: one workgroup per upper tile counts the digits of the elements that
//                                         share the prefix found so far (integer atomics: counting does not depend on the order); one
//                                         workgroup per slab scans the 256 bins from the top, extends the prefix by the digit that holds
//                                         the rank, and empties the bins.  No sort: sort_wide.h's keys are 32 bits, the threshold must be exact
//   corrw_count_kernel                    one workgroup per row: the entries >= th
//   corrw_order_kernel                    one workgroup per slab: place of feature i = the features with a larger count + the earlier ones
//                                         with an equal count; the number of features whose count is not zero
// Integer work throughout behind the Gram product: bit-reproducible, and no loop depends on the data.
#pragma once
#include "eigvals_wide.h"
#include "sort_wide.h"

namespace uglad {

constexpr int kCorrwBits = 8, kCorrwBins = 1 << kCorrwBits, kCorrwPasses = 64 / kCorrwBits;
static_assert(kCorrwBins == kWThreads, "thread = bin");

// the selection's state, in the slab's scratch area R behind the eigensolver's partials and flags (EigwView::behind_flags); 8-byte aligned
struct CorrwSel {
  unsigned long long prefix;  // the digits found so far, in place; after the last pass the pattern of th
  int rank;                   // the rank wanted among the elements that share the prefix, from the top
  int pad;
  int bins[kCorrwBins];
};
static_assert(sizeof(CorrwSel) <= 8 * kEigwSpare, "the state fits what R keeps behind the flags");
__host__ __device__ inline CorrwSel* corrw_sel(const EigwView& v, int t) { return reinterpret_cast<CorrwSel*>(v.behind_flags(t)); }
__device__ __forceinline__ unsigned long long corrw_key(double x) {
  const double a = fabs(x);
  unsigned long long key;
  __builtin_memcpy(&key, &a, sizeof(key));
  return key;
}

// grid (K)
__global__ __launch_bounds__(kWThreads) void corrw_init_kernel(int rank, EigwView v) {
  CorrwSel* s = corrw_sel(v, blockIdx.x);
  s->bins[threadIdx.x] = 0;
  if (threadIdx.x == 0) s->prefix = 0ull, s->rank = rank, s->pad = 0;
}

// grid (DP / 64, DP / 64, K); tiles below the diagonal return.  pass 0 .. 7 from the most significant digit
__global__ __launch_bounds__(kWThreads) void corrw_hist_kernel(int pass, int D, EigwView v) {
  __shared__ int s_bins[kCorrwBins];
  const int I = blockIdx.y, J = blockIdx.x, t = blockIdx.z;
  if (I > J) return;  // (uniform per workgroup)
  const int tid = threadIdx.x, DP = v.DP, shift = 64 - kCorrwBits * (pass + 1);
  CorrwSel* sel = corrw_sel(v, t);
  const unsigned long long prefix = sel->prefix;
  const double* A = v.a(t);
  s_bins[tid] = 0;
  __syncthreads();
  t64_for_each_element([&](int x, int y) {
    const int i = I * kT64 + x, j = J * kT64 + y;
    if (i >= j || j >= D) return;
    const unsigned long long key = corrw_key(A[(size_t)i * DP + j]);
    const bool shares = pass == 0 || ((key ^ prefix) >> (shift + kCorrwBits)) == 0ull;
    if (shares) atomicAdd(&s_bins[(int)((key >> shift) & (kCorrwBins - 1))], 1);
  });
  __syncthreads();
  if (s_bins[tid]) atomicAdd(&sel->bins[tid], s_bins[tid]);
}

// grid (K): thread = bin, from the top
__global__ __launch_bounds__(kWThreads) void corrw_narrow_kernel(int pass, EigwView v) {
  __shared__ int s_w[4];
  const int tid = threadIdx.x, bin = kCorrwBins - 1 - tid, shift = 64 - kCorrwBits * (pass + 1);
  CorrwSel* sel = corrw_sel(v, blockIdx.x);
  const int c = sel->bins[bin], rank = sel->rank;
  const int above = sortw_block_scan<false>(c, s_w);
  __syncthreads();  // (every thread has read the rank)
  sel->bins[bin] = 0;
  if (above <= rank && rank < above + c) {  // (one thread: the bins above hold `above` elements)
    sel->prefix |= (unsigned long long)bin << shift;
    sel->rank = rank - above;
  }
}

// grid (D, K): counts[t][i] = the entries of row i of |cov2|, zero diagonal, that are >= th
__global__ __launch_bounds__(kWThreads) void corrw_count_kernel(int D, EigwView v, int* __restrict__ counts) {
  __shared__ int s_w[4];
  const int i = blockIdx.x, t = blockIdx.y;
  const unsigned long long th = corrw_sel(v, t)->prefix;
  const double* row = v.a(t) + (size_t)i * v.DP;
  int c = 0;
  for (int j = threadIdx.x; j < D; j += kWThreads) c += (j == i ? 0ull : corrw_key(row[j])) >= th ? 1 : 0;
  c = sortw_block_sum(c, s_w);
  if (threadIdx.x == 0) counts[(size_t)t * D + i] = c;
}

// grid (K): order[t][place] = i; n_listed[t] = the features with a count above zero
__global__ __launch_bounds__(kWThreads) void corrw_order_kernel(int D, const int* __restrict__ counts, int* __restrict__ order, int* __restrict__ n_listed) {
  __shared__ int s_c[kNsMaxD];
  __shared__ int s_w[4];
  const int t = blockIdx.x, tid = threadIdx.x;
  const int* c = counts + (size_t)t * D;
  int listed = 0;
  for (int i = tid; i < D; i += kWThreads) {
    s_c[i] = c[i];
    listed += c[i] > 0 ? 1 : 0;
  }
  listed = sortw_block_sum(listed, s_w);  // (its barriers publish s_c)
  if (tid == 0) n_listed[t] = listed;
  for (int i = tid; i < D; i += kWThreads) {
    const int ci = s_c[i];
    int place = 0;
    for (int k = 0; k < D; ++k) place += (s_c[k] > ci || (s_c[k] == ci && k < i)) ? 1 : 0;
    order[(size_t)t * D + place] = i;
  }
}

}  // namespace uglad
