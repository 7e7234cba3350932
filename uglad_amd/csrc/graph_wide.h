// The recovered graph of a precision matrix (uglad_graph_wide: every 2 <= D <= the cell's own limit), many workgroups per problem: the sparsity
// threshold, the signed weighted edge list in the reference's order, node degrees and the statistics the reference prints for a graph
// (graph_from_partial_correlations, main.py:825-946, and the first six columns of compute_graph_statistics, main.py:1263-1300, which there
// are a Python double loop over D^2 entries feeding a networkx graph one edge at a time).  Definitions, all deciding and counting exactly:
//   edges = the strict upper triangle in row-major order, E = D (D - 1) / 2; the value of edge (i, j), i < j, is read at [i][j]:
//   rho_ij itself, or from a precision matrix  -P[i][j] / sqrtf(P[i][i] * P[j][j])  -- three correctly rounded fp32 operations
//   th = s[E - n_keep] with s = |rho| over the edges in ascending order (s[0] for n_keep = 0: the reference's rho_upper[-0]), or given
//   edge (i, j) is kept iff rho_ij > th or rho_ij < -th (floats, both strict: a NaN threshold keeps nothing, a NaN rho is no edge)
//   A = the 0/1 adjacency, d_i its row sums, t_i = sum_j A_ij (A A)_ij = twice the triangles at node i
//
//   gw_keys_kernel       one workgroup per 64 x 64 tile of the upper triangle, as metrics_wide.h's mw_keys_kernel: the key bits(rho) & 0x7fffffff at the edge's
//                        row-major index (|NaN| sorts last, as numpy sorts it)
//   8 x { sortw_hist_kernel, sortw_scan_kernel, sortw_scatter_kernel }     the radix sort of sort_wide.h (launch_sortw)
//   gw_threshold_kernel  one thread per problem: th from the sorted keys, or the given one (n_keep = -1)
//   gw_row_kernel        one workgroup per row of the padded plane: membership from the symmetric read [min(i, j)][max(i, j)] (A is exactly
//                        symmetric), row i of A as fp32 0/1 (leading dimension and row count padded to 64, zero-filled), d_i, the kept j > i
//                        and the row's count in each block of 64 columns
//   gw_scan_kernel       one workgroup per problem: exclusive scan of the upper counts over the rows (row offsets, m) and the 64 x 64 tile counts
//   gw_edges_kernel      one workgroup per row: its kept (i, j, rho_ij) at the row's offset in j order (block scan of the row)
//   gw_triangles_kernel  one workgroup per 64 x 64 tile (I, J) of (A A) o A, never materialising A A: a tile whose own A tile is empty leaves at
//                        once (its mask is zero; the test is uniform per workgroup), the others accumulate A[I, c] A[J, c]^T over the blocks c
//                        where both operands hold an edge, four waves with one 32 x 32 accumulator of v_mfma_f32_32x32x2_f32 each, operands
//                        staged through LDS as in wide_gemm_kernel; the accumulators are masked with the A tile and row-reduced to one int32
//                        per (row, tile column).  Every count is <= D^2 <= 2^22: exact in fp32
//   gw_rowsum_kernel     t_i = the row's partials in tile-column order
//   gw_finish_kernel     one workgroup per problem: num_nodes, num_edges, avg_degree, density, avg_clustering, transitivity as networkx
//                        computes them -- one fp64 division of exact integers each, the c_i summed in node order by one thread
//
// No atomics, no ballot, every sum in a fixed order, every buffer belongs to one problem: results are bit-reproducible and independent of K and
// of the problem's place in the batch.  One linear chain of launches, no host readback.
//
// Over the edge lists of K = R problems (uglad_edge_frequency: the selection frequencies of stability selection; at the end of this file):
//   gw_frequency_kernel         one thread per listed edge: count[i][j], count[j][i] += 1, and positive[..] where the weight is > 0 -- the
//                               file's only atomics, on integers, whose sums do not depend on their order
//   gw_frequency_totals_kernel  one workgroup: sum_{i < j} c_ij and sum_{i < j} c_ij (R - c_ij) in 64-bit integers
#pragma once
#include "sort_wide.h"

namespace uglad {

constexpr int kGwTile = kWT;    // tile of the plane: of the keys, the counts and the triangle product
constexpr int kGwKeepPer = 64;  // problems per launch of gw_threshold_kernel: their n_keep travel by value
struct GwKeep {
  int n[kGwKeepPer];
};

// One problem's part of the workspace in 4-byte words, every part even:
//   keys 0 | keys 1 | hist     the sort's part (SortwView, sort_wide.h)
//   th       2                 the threshold (float), m (int)
//   upper    DP                kept j > i of row i, then their exclusive scan
//   tile     nt x nt           edges in the 64 x 64 tile of A
//   rowtile  DP x nt           edges of row i in column block J
//   tpart    DP x nt           row i's part of t_i from tile column J
//   adj      DP x DP           A, fp32 0/1
__host__ __device__ constexpr size_t gw_tile_words(size_t nt) { return (nt * nt + 1) & ~(size_t)1; }
__host__ __device__ constexpr size_t gw_problem_words(size_t E, size_t tiles, size_t nt, size_t DP) {
  return sortw_words(E, tiles) + 2 + DP + gw_tile_words(nt) + 2 * DP * nt + DP * DP;
}
struct GwView {
  SortwView s;
  int nt, D, DP;
  __host__ __device__ size_t tile_words() const { return gw_tile_words((size_t)nt); }
  __host__ __device__ int* base(int k) const { return s.behind(k); }
  __host__ __device__ float* th(int k) const { return reinterpret_cast<float*>(base(k)); }
  __host__ __device__ int* upper(int k) const { return base(k) + 2; }
  __host__ __device__ int* tile(int k) const { return upper(k) + DP; }
  __host__ __device__ int* rowtile(int k) const { return tile(k) + tile_words(); }
  __host__ __device__ int* tpart(int k) const { return rowtile(k) + (size_t)DP * nt; }
  __host__ __device__ float* adj(int k) const { return reinterpret_cast<float*>(tpart(k) + (size_t)DP * nt); }
};
__host__ inline GwView gw_view(float* workspace, int D) {
  const int E = D * (D - 1) / 2, tiles = sortw_tiles(E), nt = (D + kGwTile - 1) / kGwTile, DP = nt * kGwTile;
  return GwView{SortwView{reinterpret_cast<unsigned*>(workspace), gw_problem_words((size_t)E, (size_t)tiles, (size_t)nt, (size_t)DP), E, tiles}, nt, D, DP};
}
__host__ inline size_t gw_problem_floats(int D) { return gw_view(nullptr, D).s.stride; }

// the value of edge (i, j), i < j
__device__ __forceinline__ float gw_rho(const float* __restrict__ Vm, int D, int i, int j, int from_precision) {
  const float x = Vm[(size_t)i * D + j];
  if (!from_precision) return x;
  return -x / sqrtf(Vm[(size_t)i * D + i] * Vm[(size_t)j * D + j]);
}

// ---------------------------------------------------------------------------------------------------------------- keys
// grid (nt, nt, K): tile (I, J) = (blockIdx.y, blockIdx.x) of 64 x 64; tiles below the diagonal hold no edge
__global__ __launch_bounds__(kWThreads) void gw_keys_kernel(const float* __restrict__ values, int from_precision, GwView v) {
  const int I = blockIdx.y, J = blockIdx.x, k = blockIdx.z, tid = threadIdx.x, D = v.D;
  if (I > J) return;  // (uniform per workgroup)
  const float* Vm = values + (size_t)k * D * D;
  unsigned* keys = v.s.keys(k, 0);
  const int j = J * kGwTile + (tid & 63);
  for (int r = tid >> 6; r < kGwTile; r += 4) {
    const int i = I * kGwTile + r;
    if (i < j && j < D) keys[i * D - (i * (i + 1)) / 2 + (j - i - 1)] = (unsigned)__float_as_int(gw_rho(Vm, D, i, j, from_precision)) & 0x7fffffffu;
  }
}

// ---------------------------------------------------------------------------------------------------------------- threshold
// grid (problems of this launch), one thread each: problem k0 + blockIdx.x
__global__ void gw_threshold_kernel(GwKeep keep, int k0, const float* __restrict__ threshold_in, float* __restrict__ threshold, GwView v) {
  if (threadIdx.x != 0) return;
  const int k = k0 + blockIdx.x, n = keep.n[blockIdx.x];
  const float th = n < 0 ? threshold_in[k] : __int_as_float((int)v.s.keys(k, 0)[n == 0 ? 0 : v.s.E - n]);
  v.th(k)[0] = th;
  threshold[k] = th;
}

// ---------------------------------------------------------------------------------------------------------------- rows of A
// grid (DP, K): row i of the padded plane (rows i >= D are zero)
__global__ __launch_bounds__(kWThreads) void gw_row_kernel(const float* __restrict__ values, int from_precision, int* __restrict__ degree,
                                                           GwView v) {
  __shared__ int s_w[4];
  const int i = blockIdx.x, k = blockIdx.y, tid = threadIdx.x, D = v.D, DP = v.DP;
  const float* Vm = values + (size_t)k * D * D;
  float* arow = v.adj(k) + (size_t)i * DP;
  int* rt = v.rowtile(k) + (size_t)i * v.nt;
  const float th = v.th(k)[0];
  int deg = 0, up = 0;
  for (int j0 = 0; j0 < DP; j0 += kWThreads) {
    const int j = j0 + tid;  // (DP is a multiple of 64: a wave is inside the plane or outside as a whole, and covers one column block)
    if (j >= DP) continue;
    int e = 0;
    if (i < D && j < D && j != i) {
      const float rho = gw_rho(Vm, D, i < j ? i : j, i < j ? j : i, from_precision);
      e = (rho > th || rho < -th) ? 1 : 0;
    }
    arow[j] = e ? 1.f : 0.f;
    int c = e;
    for (int m = 32; m >= 1; m >>= 1) c += __shfl_xor(c, m);
    if ((tid & 63) == 0) rt[j >> 6] = c;
    deg += e;
    up += (e && j > i) ? 1 : 0;
  }
  deg = sortw_block_sum(deg, s_w);
  up = sortw_block_sum(up, s_w);
  if (tid == 0) {
    v.upper(k)[i] = up;
    if (i < D) degree[(size_t)k * D + i] = deg;
  }
}

// grid (K): upper -> its exclusive scan over the rows (where row i's edges start), m; the tile counts
__global__ __launch_bounds__(kWThreads) void gw_scan_kernel(int* __restrict__ edge_count, GwView v) {
  __shared__ int s_w[4];
  const int k = blockIdx.x, tid = threadIdx.x, nt = v.nt;
  int* h = v.upper(k);
  const int n = v.DP, per = (n + kWThreads - 1) / kWThreads;
  const int lo = tid * per < n ? tid * per : n, hi = lo + per < n ? lo + per : n;
  int s = 0;
  for (int q = lo; q < hi; ++q) s += h[q];
  int run = sortw_block_scan<false>(s, s_w);
  for (int q = lo; q < hi; ++q) {
    const int c = h[q];
    h[q] = run;
    run += c;
  }
  if (tid == kWThreads - 1) {  // (the last thread's range ends the rows: run = m)
    reinterpret_cast<int*>(v.th(k))[1] = run;
    edge_count[k] = run;
  }
  const int* rt = v.rowtile(k);
  int* tc = v.tile(k);
  for (int t = tid; t < nt * nt; t += kWThreads) {
    const int I = t / nt, J = t - I * nt;
    int c = 0;
    for (int r = 0; r < kGwTile; ++r) c += rt[(size_t)(I * kGwTile + r) * nt + J];
    tc[t] = c;
  }
}

// ---------------------------------------------------------------------------------------------------------------- edge list
// grid (D, K): row i writes its kept (i, j, rho_ij), j > i ascending, from upper[i] on
__global__ __launch_bounds__(kWThreads) void gw_edges_kernel(const float* __restrict__ values, int from_precision, int* __restrict__ edge_ij,
                                                             float* __restrict__ edge_w, GwView v) {
  __shared__ int s_w[4];
  const int i = blockIdx.x, k = blockIdx.y, tid = threadIdx.x, D = v.D;
  const float* Vm = values + (size_t)k * D * D;
  const float* arow = v.adj(k) + (size_t)i * v.DP;
  int run = v.upper(k)[i];
  for (int j0 = i + 1; j0 < D; j0 += kWThreads) {  // (uniform per workgroup)
    const int j = j0 + tid;
    const int e = (j < D && arow[j] != 0.f) ? 1 : 0;
    const int before = sortw_block_scan<false>(e, s_w);
    const int total = (s_w[0] + s_w[1]) + (s_w[2] + s_w[3]);  // (the waves' totals, left by the scan; its next call starts with a barrier)
    if (e) {
      const size_t at = (size_t)k * v.s.E + (size_t)(run + before);
      edge_ij[2 * at] = i;
      edge_ij[2 * at + 1] = j;
      edge_w[at] = gw_rho(Vm, D, i, j, from_precision);
    }
    run += total;
  }
}

// ---------------------------------------------------------------------------------------------------------------- triangles
// grid (nt, nt, K): tile (I, J) = (blockIdx.y, blockIdx.x) of (A A) o A -> tpart[row][J] for the 64 rows of I
__global__ __launch_bounds__(kWThreads) void gw_triangles_kernel(GwView v) {
  __shared__ float sA[kWK * kWLd], sB[kWK * kWLd];
  static_assert(kWK == kGwTile, "one tile size for the plane, the counts and the product");
  const int I = blockIdx.y, J = blockIdx.x, k = blockIdx.z, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int nt = v.nt, DP = v.DP;
  const int* tc = v.tile(k);
  int* part = v.tpart(k) + (size_t)(I * kWT) * nt + J;
  if (tc[I * nt + J] == 0) {  // (uniform per workgroup) the mask is zero
    if (tid < kWT) part[(size_t)tid * nt] = 0;
    return;
  }
  const float* A = v.adj(k);
  const float* Ai = A + (size_t)(I * kWT) * DP;
  const float* Aj = A + (size_t)(J * kWT) * DP;
  f32x16 acc;
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.f;
  const int wi = (w >> 1) * 32, wj = (w & 1) * 32, li = lane & 31, kh = lane >> 5;
  for (int c = 0; c < nt; ++c) {
    if (tc[I * nt + c] == 0 || tc[J * nt + c] == 0) continue;  // (uniform per workgroup) a zero operand
    __syncthreads();                                           // (the previous chunk has been consumed)
#pragma unroll
    for (int pp = 0; pp < kWT / 4; ++pp) {  // a wave reads 64 consecutive k of one row; [k][x] in LDS: conflict-free both ways
      const int r = w + 4 * pp;
      sA[lane * kWLd + r] = Ai[(size_t)r * DP + c * kWK + lane];
      sB[lane * kWLd + r] = Aj[(size_t)r * DP + c * kWK + lane];
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < kWK / 2; ++u) {
      const int kk = 2 * u + kh;
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(sA[kk * kWLd + wi + li], sB[kk * kWLd + wj + li], acc, 0, 0, 0);
    }
  }
  // accumulator entry e of lane l = C[wi + acc_row(e, l)][wj + (l & 31)]: masked, through LDS, one thread per row
  __syncthreads();
  float* sC = sA;
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int r = wi + acc_row(e, lane);
    sC[r * kWLd + wj + li] = acc[e] * Ai[(size_t)r * DP + J * kWT + wj + li];
  }
  __syncthreads();
  if (tid < kWT) {
    float s = 0.f;
    for (int c = 0; c < kWT; ++c) s += sC[tid * kWLd + c];  // (integers <= 64 D: exact)
    part[(size_t)tid * nt] = (int)s;
  }
}

// grid (ceil(D / 256), K)
__global__ __launch_bounds__(kWThreads) void gw_rowsum_kernel(int* __restrict__ triangles2, GwView v) {
  const int i = blockIdx.x * kWThreads + threadIdx.x, k = blockIdx.y, nt = v.nt;
  if (i >= v.D) return;
  const int* part = v.tpart(k) + (size_t)i * nt;
  int t = 0;
  for (int J = 0; J < nt; ++J) t += part[J];
  triangles2[(size_t)k * v.D + i] = t;
}

// ---------------------------------------------------------------------------------------------------------------- the six numbers
// grid (K).  The four sums run side by side, one thread each, over chunks of 256 nodes staged in LDS: sum d_i, sum d_i (d_i - 1) and sum t_i
// are integers below 2^53 -- exact as doubles in any order --, the c_i are added in node order (entries past D are +0.0: they change nothing).
__global__ __launch_bounds__(kWThreads) void gw_finish_kernel(const int* __restrict__ degree, const int* __restrict__ triangles2,
                                                              double* __restrict__ stats, GwView v) {
  constexpr int kRow = kWThreads + 1;
  __shared__ double s_v[4 * kRow], s_sum[4];
  const int k = blockIdx.x, tid = threadIdx.x, D = v.D;
  const int* deg = degree + (size_t)k * D;
  const int* tri = triangles2 + (size_t)k * D;
  double sum = 0.0;  // of thread tid < 4: sum d_i, sum d_i (d_i - 1), sum t_i, sum c_i
  for (int i0 = 0; i0 < D; i0 += kWThreads) {
    __syncthreads();
    const int i = i0 + tid;
    const long long d = i < D ? deg[i] : 0, t = i < D ? tri[i] : 0;
    s_v[tid] = (double)d;
    s_v[kRow + tid] = (double)(d * (d - 1));
    s_v[2 * kRow + tid] = (double)t;
    s_v[3 * kRow + tid] = t == 0 ? 0.0 : (double)t / (double)(d * (d - 1));
    __syncthreads();
    if (tid < 4) {
#pragma unroll 8
      for (int q = 0; q < kWThreads; ++q) sum += s_v[tid * kRow + q];
    }
  }
  if (tid < 4) s_sum[tid] = sum;
  __syncthreads();
  if (tid == 0) {
    const double n = (double)D, m = (double)reinterpret_cast<const int*>(v.th(k))[1];
    double* o = stats + (size_t)k * 6;
    o[0] = n;
    o[1] = m;
    o[2] = s_sum[0] / n;
    o[3] = m / (double)((long long)D * (D - 1)) * 2.0;
    o[4] = s_sum[3] / n;
    o[5] = s_sum[2] == 0.0 ? 0.0 : s_sum[2] / s_sum[1];
  }
}

// ---------------------------------------------------------------------------------------------------------------- edge frequencies
// uglad_edge_frequency: how often every edge comes back over the R edge lists gw_edges_kernel leaves for K = R problems (the selection
// frequencies of stability selection).  grid (ceil(E / 256), R), one thread per listed edge: the first edge_count[r] rows of list r, the
// rest of a list is undefined and never read.  count[i][j] and count[j][i] += 1, positive[..] += 1 where the weight is > 0, on planes the
// entry point has zeroed.  Integer atomics: the sums do not depend on their order.  An index outside the plane is skipped, not stored.
__global__ __launch_bounds__(kWThreads) void gw_frequency_kernel(const int* __restrict__ edge_count, const int* __restrict__ edge_ij,
                                                                 const float* __restrict__ edge_w, int E, int D, int* __restrict__ count,
                                                                 int* __restrict__ positive) {
  const int r = blockIdx.y, e = blockIdx.x * kWThreads + threadIdx.x;
  if (e >= E || e >= edge_count[r]) return;
  const size_t at = (size_t)r * E + e;
  const int i = edge_ij[2 * at], j = edge_ij[2 * at + 1];
  if (i < 0 || j < 0 || i >= D || j >= D || i == j) return;
  atomicAdd(count + (size_t)i * D + j, 1);
  atomicAdd(count + (size_t)j * D + i, 1);
  if (edge_w[at] > 0.f) {
    atomicAdd(positive + (size_t)i * D + j, 1);
    atomicAdd(positive + (size_t)j * D + i, 1);
  }
}

// grid (1): totals = {sum_{i < j} c_ij, sum_{i < j} c_ij (R - c_ij)} in 64-bit integers -- row i's columns j > i strided over the threads,
// the 256 partial sums combined by thread 0 (integers: any order gives the same bits).  StARS' instability is 2 totals[1] / (R^2 E).
__global__ __launch_bounds__(kWThreads) void gw_frequency_totals_kernel(const int* __restrict__ count, int R, int D, long long* __restrict__ totals) {
  __shared__ long long s_a[kWThreads], s_b[kWThreads];
  const int tid = threadIdx.x;
  long long a = 0, b = 0;
  for (int i = 0; i < D; ++i)
    for (int j = i + 1 + tid; j < D; j += kWThreads) {
      const long long c = count[(size_t)i * D + j];
      a += c;
      b += c * ((long long)R - c);
    }
  s_a[tid] = a;
  s_b[tid] = b;
  __syncthreads();
  if (tid != 0) return;
  for (int k = 1; k < kWThreads; ++k) a += s_a[k], b += s_b[k];
  totals[0] = a;
  totals[1] = b;
}

}  // namespace uglad
