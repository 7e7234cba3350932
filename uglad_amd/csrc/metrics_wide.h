// Support-recovery metrics beyond the one-workgroup kernel's size (uglad_support_metrics_wide: every 2 <= D <= the cell's own limit), many
// workgroups per (true, predicted) pair.  after_path.h's support_metrics_kernel keeps all E = D (D - 1) / 2 scores of a pair in the LDS of one
// workgroup and sweeps them once per true edge (O(T E)); here the edges are SORTED by score, after which every quantity of the ranking
// metrics is a prefix count: O(E) work per pass of the sort, whatever the labels.  Same definitions, all counting in integers:
//   edges = the strict upper triangle; label = true != 0, prediction = pred != 0 (both decided on the bit pattern, (bits & 0x7fffffff) != 0:
//   denormals and -0.0 behave as in numpy whatever the flush mode); score = |pred|
//   AUC = MW2 / (2 T F), MW2 = sum over true edges of 2 #(false edges with a smaller score) + #(false edges with an equal score)
//   AP  = (1 / T) sum over true edges of #(true edges with score >= s) / #(edges with score >= s);   both NaN when T = 0 or F = 0
//
//   mw_keys_kernel      one workgroup per 64 x 64 tile of the upper triangle (rows of the tile read along j): one 32-bit key per edge,
//                       ((bits(pred) & 0x7fffffff) << 1) | label -- the sign bit of |x| is free, so unsigned key order is (score, label) order
//                       and the positives close every tie group -- stored at the edge's row-major index; and the tile's counts T, P, TP
//   8 x { sortw_hist_kernel, sortw_scan_kernel, sortw_scatter_kernel }
//                       the radix sort of sort_wide.h on the keys of each pair (launch_sortw); every 32-bit value is a legal key
//                       (0xffffffff = |NaN|, label 1)
//   mw_chunk_kernel     per 2048 sorted keys: the positives in the chunk, its last group boundary (where key >> 1 changes) and the positives
//                       of the chunk in front of that boundary
//   mw_group_kernel     per chunk: what lies in front of it from the chunk records (positives; the start a of the tie group that reaches into
//                       the chunk and pos[0, a)), then every true edge at sorted index g, in a group that starts at a, adds
//                         (a - pos[0, a)) + (g - pos[0, g))  =  2 negBelow + (negatives of its group: they all sit in front of g)    to MW2
//                         (T - pos[0, a)) / (E - a)          =  posGE / allGE                                                        to AP
//                       MW2 in int64, AP in fp64, thread order inside the chunk
//   mw_finish_kernel    one workgroup per pair: the counts; MW2 and AP over the chunks in index order; the 11 doubles by the expressions of
//                       support_metrics_kernel's last block (identical IEEE operations: everything but aupr is bit-equal to it)
//
// aupr differs from the one-workgroup kernel in the order of its T terms only.  Every sum has a fixed order and every buffer belongs to one
// pair: results are bit-reproducible and independent of K and of the pair's place and neighbours in the batch.  NaN scores (sklearn raises on
// them) sort by their bit pattern above every finite score; the call terminates and returns what that order gives.
// 4 + 3 x 8 launches in one linear chain, no host readback.
#pragma once
#include "sort_wide.h"

namespace uglad {

constexpr int kMwKeyTile = 64;  // tile of the upper triangle in mw_keys_kernel

// One pair's part of the workspace in 4-byte words (the buffer is 8-byte aligned and every part even, so the 64-bit parts stay aligned):
//   keys 0 | keys 1 | hist   the sort's part (SortwView, sort_wide.h)
//   kpart  nt x nt x 4  T, P, TP of every tile of mw_keys_kernel
//   chunk  tiles x 4    positives, last boundary (-1: none), positives in front of it
//   mw2    tiles int64 | ap   tiles fp64
struct MwView {
  SortwView s;
  int nt;
  __host__ __device__ int* kpart(int k) const { return s.behind(k); }
  __host__ __device__ int* chunk(int k) const { return kpart(k) + 4 * (size_t)nt * nt; }
  __host__ __device__ long long* mw2(int k) const { return reinterpret_cast<long long*>(chunk(k) + 4 * (size_t)s.tiles); }
  __host__ __device__ double* ap(int k) const { return reinterpret_cast<double*>(mw2(k) + s.tiles); }
};
__host__ __device__ constexpr size_t mw_pair_words(size_t E, size_t tiles, size_t nt) {
  return sortw_words(E, tiles) + 4 * nt * nt + 4 * tiles + 2 * tiles + 2 * tiles;
}
__host__ inline MwView mw_view(float* workspace, int D) {
  const int E = D * (D - 1) / 2, tiles = sortw_tiles(E), nt = (D + kMwKeyTile - 1) / kMwKeyTile;
  return MwView{SortwView{reinterpret_cast<unsigned*>(workspace), mw_pair_words((size_t)E, (size_t)tiles, (size_t)nt), E, tiles}, nt};
}
__host__ inline size_t mw_pair_floats(int D) { return mw_view(nullptr, D).s.stride; }

// ---------------------------------------------------------------------------------------------------------------- keys and counts
// grid (nt, nt, K): tile (I, J) = (blockIdx.y, blockIdx.x) of 64 x 64; tiles below the diagonal only zero their counts
__global__ __launch_bounds__(kWThreads) void mw_keys_kernel(const float* __restrict__ true_theta, const float* __restrict__ pred_theta, int D,
                                                            MwView v) {
  __shared__ int s_w[4];
  const int I = blockIdx.y, J = blockIdx.x, k = blockIdx.z, tid = threadIdx.x;
  int* part = v.kpart(k) + 4 * (I * v.nt + J);
  if (I > J) {  // (uniform per workgroup)
    if (tid < 4) part[tid] = 0;
    return;
  }
  const size_t base = (size_t)k * D * D;
  unsigned* keys = v.s.keys(k, 0);
  const int j = J * kMwKeyTile + (tid & 63);
  int n_true = 0, n_pred = 0, n_both = 0;
  for (int r = tid >> 6; r < kMwKeyTile; r += 4) {
    const int i = I * kMwKeyTile + r;
    if (i < j && j < D) {
      const size_t at = base + (size_t)i * D + j;
      const unsigned mag = (unsigned)__float_as_int(pred_theta[at]) & 0x7fffffffu;
      const unsigned label = ((unsigned)__float_as_int(true_theta[at]) & 0x7fffffffu) != 0u;
      keys[i * D - (i * (i + 1)) / 2 + (j - i - 1)] = (mag << 1) | label;
      n_true += (int)label;
      n_pred += mag != 0u;
      n_both += label && mag != 0u;
    }
  }
  n_true = sortw_block_sum(n_true, s_w);
  n_pred = sortw_block_sum(n_pred, s_w);
  n_both = sortw_block_sum(n_both, s_w);
  if (tid == 0) part[0] = n_true, part[1] = n_pred, part[2] = n_both, part[3] = 0;
}

// ---------------------------------------------------------------------------------------------------------------- group statistics
// what a thread sees in its kSortwPer sorted keys: positives, the last group boundary (index in the thread, -1: none) and the positives in front of it
struct MwRun {
  int npos, last, pos_before_last;
  unsigned bounds;  // bit j: key j starts a tie group
};
__device__ __forceinline__ MwRun mw_run(const unsigned* __restrict__ keys, const unsigned (&key)[kSortwPer], int n, int g0) {
  MwRun r{0, -1, 0, 0u};
  unsigned prev = (n > 0 && g0 > 0) ? keys[g0 - 1] : 0u;
#pragma unroll
  for (int j = 0; j < kSortwPer; ++j)
    if (j < n) {
      if (g0 + j == 0 || (key[j] >> 1) != (prev >> 1)) r.bounds |= 1u << j, r.last = j, r.pos_before_last = r.npos;
      r.npos += (int)(key[j] & 1u);
      prev = key[j];
    }
  return r;
}

// grid (tiles, K): the chunk's record
__global__ __launch_bounds__(kWThreads) void mw_chunk_kernel(MwView v) {
  __shared__ int s_w[4];
  const int c = blockIdx.x, k = blockIdx.y, tid = threadIdx.x;
  const unsigned* keys = v.s.keys(k, 0);
  unsigned key[kSortwPer];
  const int n = sortw_load(keys, v.s.E, c, key);
  const MwRun r = mw_run(keys, key, n, c * kSortwTile + tid * kSortwPer);
  const int before = sortw_block_scan<false>(r.npos, s_w);
  const int owner = sortw_block_max(r.last >= 0 ? tid : -1, s_w);  // the last thread that holds a boundary
  int* rec = v.chunk(k) + 4 * c;
  if (tid == kWThreads - 1) rec[0] = before + r.npos, rec[3] = 0;
  if (owner < 0 && tid == 0) rec[1] = -1, rec[2] = 0;
  if (tid == owner) rec[1] = tid * kSortwPer + r.last, rec[2] = before + r.pos_before_last;
}

// grid (tiles, K): the chunk's share of MW2 and of the sum of AP
__global__ __launch_bounds__(kWThreads) void mw_group_kernel(MwView v) {
  __shared__ int s_w[4], s_a[kWThreads], s_pa[kWThreads];
  __shared__ long long s_mw[kWThreads];
  __shared__ double s_ap[kWThreads];
  const int c = blockIdx.x, k = blockIdx.y, tid = threadIdx.x;
  const int* rec = v.chunk(k);
  // in front of the chunk: the positives, and the last chunk with a boundary (chunk 0 starts a group: there is one for every c > 0)
  int pos_in = 0, all = 0, cb = -1;
  for (int q = tid; q < v.s.tiles; q += kWThreads) {
    const int np = rec[4 * q];
    all += np;
    if (q < c) {
      pos_in += np;
      if (rec[4 * q + 1] >= 0) cb = q;
    }
  }
  pos_in = sortw_block_sum(pos_in, s_w);
  const int T = sortw_block_sum(all, s_w);
  cb = sortw_block_max(cb, s_w);
  int a_in = 0, pa_in = 0;  // start of the group that reaches into the chunk and the positives in front of that start
  if (cb >= 0) {            // (uniform per workgroup)
    int s = 0;
    for (int q = tid; q < cb; q += kWThreads) s += rec[4 * q];
    a_in = cb * kSortwTile + rec[4 * cb + 1];
    pa_in = sortw_block_sum(s, s_w) + rec[4 * cb + 2];
  }
  const unsigned* keys = v.s.keys(k, 0);
  unsigned key[kSortwPer];
  const int n = sortw_load(keys, v.s.E, c, key);
  const int g0 = c * kSortwTile + tid * kSortwPer;
  const MwRun r = mw_run(keys, key, n, g0);
  int pos = pos_in + sortw_block_scan<false>(r.npos, s_w);  // positives in front of the thread's first key
  s_a[tid] = g0 + r.last;
  s_pa[tid] = pos + r.pos_before_last;
  const int owner = sortw_block_scan<true>(r.last >= 0 ? tid : -1, s_w);  // (its barriers publish s_a / s_pa) the last earlier thread with a boundary
  int a = owner >= 0 ? s_a[owner] : a_in, pa = owner >= 0 ? s_pa[owner] : pa_in;
  long long mw = 0;
  double ap = 0.0;
#pragma unroll
  for (int j = 0; j < kSortwPer; ++j)
    if (j < n) {
      if ((r.bounds >> j) & 1u) a = g0 + j, pa = pos;
      if (key[j] & 1u) {
        mw += (long long)(a - pa) + (long long)(g0 + j - pos);
        ap += (double)(T - pa) / (double)(v.s.E - a);
        ++pos;
      }
    }
  s_mw[tid] = mw;
  s_ap[tid] = ap;
  __syncthreads();
  if (tid == 0) {
    long long m = 0;
    double s = 0.0;
    for (int q = 0; q < kWThreads; ++q) m += s_mw[q], s += s_ap[q];
    v.mw2(k)[c] = m;
    v.ap(k)[c] = s;
  }
}

// ---------------------------------------------------------------------------------------------------------------- the 11 numbers
// grid (K)
__global__ __launch_bounds__(kWThreads) void mw_finish_kernel(double* __restrict__ out, int beta, MwView v) {
  __shared__ int s_w[4];
  __shared__ long long s_mw[kWThreads];
  __shared__ double s_ap[kWThreads];
  const int k = blockIdx.x, tid = threadIdx.x;
  const int* part = v.kpart(k);
  int n_true = 0, n_pred = 0, n_both = 0;
  for (int q = tid; q < v.nt * v.nt; q += kWThreads) n_true += part[4 * q], n_pred += part[4 * q + 1], n_both += part[4 * q + 2];
  const long long Tn = sortw_block_sum(n_true, s_w), Pn = sortw_block_sum(n_pred, s_w), TP = sortw_block_sum(n_both, s_w);
  // the chunks' partial sums in index order: 256 at a time through LDS (one thread adds, all threads fetch)
  long long MW2 = 0;
  double AP = 0.0;
  for (int c0 = 0; c0 < v.s.tiles; c0 += kWThreads) {
    __syncthreads();
    if (c0 + tid < v.s.tiles) s_mw[tid] = v.mw2(k)[c0 + tid], s_ap[tid] = v.ap(k)[c0 + tid];
    __syncthreads();
    if (tid == 0)
      for (int q = 0; q < kWThreads && c0 + q < v.s.tiles; ++q) MW2 += s_mw[q], AP += s_ap[q];
  }
  if (tid == 0) {
    const double dTP = (double)TP, dP = (double)Pn, dT = (double)Tn, dF = (double)v.s.E - dT;
    const double FP = dP - dTP, FN = dT - dTP;
    const double b2 = (double)beta * (double)beta;
    double* o = out + (size_t)k * 11;
    o[0] = FP / dP;
    o[1] = dTP / dT;
    o[2] = FP / dF;
    o[3] = FP + FN;
    o[4] = dT;
    o[5] = dP;
    o[6] = dTP / (dTP + FP);
    o[7] = dTP / (dTP + FN);
    o[8] = (1.0 + b2) * dTP / ((1.0 + b2) * dTP + b2 * FN + FP);
    o[9] = (Tn > 0 && dF > 0) ? AP / dT : __builtin_nan("");
    o[10] = (Tn > 0 && dF > 0) ? (double)MW2 / (2.0 * dT * dF) : __builtin_nan("");
  }
}

}  // namespace uglad
