// The radix sort of the wide utilities (metrics_wide.h, graph_wide.h): K independent arrays of E 32-bit keys each, sorted ascending as
// unsigned integers, many workgroups per array.
//
//   8 x { sortw_hist_kernel, sortw_scan_kernel, sortw_scatter_kernel }     (launch_sortw, host_wide.h)
//                       least-significant-digit radix sort, 4 bits per pass, tiles of 2048 keys: the tile's 16 digit counts; their exclusive
//                       scan in (digit, tile) order, one workgroup per array; the stable scatter.  A thread holds 8 CONSECUTIVE keys and
//                       counts its digits in one 64-bit register (16 x 4 bits); the scan of the 16 x 256 counts in (digit, thread) order is
//                       the key's place in the sorted tile, the tile is sorted in LDS and leaves in runs of equal digits.
//                       No ballot, no atomics, no workgroup waits on another; every 32-bit value is a legal key and the ragged last tile is
//                       handled by its count
// and the workgroup helpers (sum, maximum, exclusive scan over 256 threads) that its kernels and its clients share.
#pragma once
#include "wide_bwd.h"

namespace uglad {

constexpr int kSortwBits = 4, kSortwBins = 1 << kSortwBits, kSortwPasses = 32 / kSortwBits;
constexpr int kSortwPer = 8;                    // consecutive keys per thread: a digit's count in a thread fits 4 bits
constexpr int kSortwTile = kWThreads * kSortwPer;  // keys per workgroup
static_assert(kWThreads == 256 && kSortwBins * kSortwBits == 64 && kSortwPer < kSortwBins, "a thread's digit counts share one 64-bit register");

// What the sort reads of an item's part of the workspace, in 4-byte words (the buffer is 8-byte aligned and every part even, so 64-bit parts
// behind it stay aligned).  Item k is `stride` words -- the CLIENT's whole part -- and begins with
//   keys 0 | keys 1   E words each, rounded up to even: the sort's two buffers (the sorted keys end in buffer 0)
//   hist   16 x tiles   digit counts of the pass, then their exclusive scan, (digit, tile) order
// and goes on as its client's layout says, from behind(k).
struct SortwView {
  unsigned* ws;
  size_t stride;  // words per item
  int E, tiles;
  __host__ __device__ size_t epad() const { return ((size_t)E + 1) & ~(size_t)1; }
  __host__ __device__ unsigned* keys(int k, int which) const { return ws + (size_t)k * stride + (size_t)which * epad(); }
  __host__ __device__ int* hist(int k) const { return reinterpret_cast<int*>(keys(k, 2)); }
  __host__ __device__ int* behind(int k) const { return hist(k) + (size_t)kSortwBins * tiles; }
};
__host__ __device__ constexpr int sortw_tiles(int E) { return (E + kSortwTile - 1) / kSortwTile; }
__host__ __device__ constexpr size_t sortw_words(size_t E, size_t tiles) { return 2 * ((E + 1) & ~(size_t)1) + kSortwBins * tiles; }

// ---------------------------------------------------------------------------------------------------------------- workgroup helpers
// (256 threads = 4 waves; s_w: 4 ints of LDS; the first barrier protects s_w's previous use)
__device__ __forceinline__ int sortw_block_sum(int v, int* s_w) {
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
  __syncthreads();
  return (s_w[0] + s_w[1]) + (s_w[2] + s_w[3]);
}
__device__ __forceinline__ int sortw_block_max(int v, int* s_w) {
  for (int m = 32; m >= 1; m >>= 1) {
    const int o = __shfl_xor(v, m);
    v = o > v ? o : v;
  }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
  __syncthreads();
  const int a = s_w[0] > s_w[1] ? s_w[0] : s_w[1], b = s_w[2] > s_w[3] ? s_w[2] : s_w[3];
  return a > b ? a : b;
}
// exclusive prefix in thread order: kMax = false the sum (identity 0), kMax = true the maximum (identity -1)
template <bool kMax>
__device__ __forceinline__ int sortw_block_scan(int v, int* s_w) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  auto op = [](int a, int b) { return kMax ? (a > b ? a : b) : a + b; };
  int inc = v;
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl(inc, lane - d);
    if (lane >= d) inc = op(inc, o);
  }
  int prev = __shfl(inc, lane - 1);  // the wave's exclusive prefix
  if (lane == 0) prev = kMax ? -1 : 0;
  __syncthreads();
  if (lane == 63) s_w[w] = inc;
  __syncthreads();
  int before = kMax ? -1 : 0;
  for (int q = 0; q < 3; ++q)
    if (q < w) before = op(before, s_w[q]);
  return op(before, prev);
}

// the thread's kSortwPer consecutive keys of tile `tile`; returns how many of them exist (the ragged tail: by count, no sentinel)
__device__ __forceinline__ int sortw_load(const unsigned* __restrict__ keys, int E, int tile, unsigned (&key)[kSortwPer]) {
  const int g0 = tile * kSortwTile + (int)threadIdx.x * kSortwPer;
  if (g0 + kSortwPer <= E) {  // (g0 is even and so is every buffer's offset: 8-byte aligned)
    __builtin_memcpy(key, __builtin_assume_aligned(keys + g0, 8), sizeof(unsigned) * kSortwPer);
    return kSortwPer;
  }
#pragma unroll
  for (int j = 0; j < kSortwPer; ++j) key[j] = g0 + j < E ? keys[g0 + j] : 0u;
  return E - g0 > 0 ? E - g0 : 0;
}
__device__ __forceinline__ int sortw_digit(unsigned key, int pass) { return (int)((key >> (kSortwBits * pass)) & (kSortwBins - 1)); }
// the thread's 16 digit counts, 4 bits each
__device__ __forceinline__ unsigned long long sortw_count(const unsigned (&key)[kSortwPer], int n, int pass) {
  unsigned long long packed = 0;
#pragma unroll
  for (int j = 0; j < kSortwPer; ++j)
    if (j < n) packed += 1ull << (kSortwBits * sortw_digit(key[j], pass));
  return packed;
}

// ---------------------------------------------------------------------------------------------------------------- one pass of the sort
// grid (tiles, K): hist[digit][tile] = keys of the tile with that digit
__global__ __launch_bounds__(kWThreads) void sortw_hist_kernel(int pass, int src, SortwView v) {
  constexpr int kRow = kWThreads + 16;  // (row stride 16 mod 64: the four digits a wave sums at once sit in different banks)
  __shared__ int s_cnt[kSortwBins * kRow];
  const int tile = blockIdx.x, k = blockIdx.y, tid = threadIdx.x;
  unsigned key[kSortwPer];
  const int n = sortw_load(v.keys(k, src), v.E, tile, key);
  const unsigned long long packed = sortw_count(key, n, pass);
#pragma unroll
  for (int d = 0; d < kSortwBins; ++d) s_cnt[d * kRow + tid] = (int)((packed >> (kSortwBits * d)) & 15);
  __syncthreads();
  // 16 threads per digit, each 16 of the 256 counts; the 16 partial sums meet by a butterfly inside the 16 lanes
  const int d = tid >> 4, seg = tid & 15;
  int s = 0;
#pragma unroll
  for (int i = 0; i < 16; ++i) s += s_cnt[d * kRow + i * 16 + seg];
  for (int m = 8; m >= 1; m >>= 1) s += __shfl_xor(s, m);
  if (seg == 0) v.hist(k)[(size_t)d * v.tiles + tile] = s;
}

// grid (K): the exclusive scan of hist in (digit, tile) order, in place: where the tile's keys with that digit go
__global__ __launch_bounds__(kWThreads) void sortw_scan_kernel(SortwView v) {
  __shared__ int s_w[4];
  int* h = v.hist(blockIdx.x);
  const int n = kSortwBins * v.tiles, per = (n + kWThreads - 1) / kWThreads;
  const int lo = (int)threadIdx.x * per < n ? (int)threadIdx.x * per : n, hi = lo + per < n ? lo + per : n;
  int s = 0;
  for (int i = lo; i < hi; ++i) s += h[i];
  int run = sortw_block_scan<false>(s, s_w);
  for (int i = lo; i < hi; ++i) {
    const int c = h[i];
    h[i] = run;
    run += c;
  }
}

// grid (tiles, K): stable scatter of the tile by the pass's digit
__global__ __launch_bounds__(kWThreads) void sortw_scatter_kernel(int pass, int src, SortwView v) {
  __shared__ int s_cnt[kSortwBins * kWThreads + kWThreads];  // entry i = (digit, thread) at i + (i >> 4): 16 consecutive entries per thread, no bank conflicts
  __shared__ unsigned s_key[kSortwTile];
  __shared__ int s_w[4], s_start[kSortwBins], s_dst[kSortwBins];
  const int tile = blockIdx.x, k = blockIdx.y, tid = threadIdx.x;
  auto at = [](int i) { return i + (i >> 4); };
  unsigned key[kSortwPer];
  const int n = sortw_load(v.keys(k, src), v.E, tile, key);
  const unsigned long long packed = sortw_count(key, n, pass);
#pragma unroll
  for (int d = 0; d < kSortwBins; ++d) s_cnt[at(d * kWThreads + tid)] = (int)((packed >> (kSortwBits * d)) & 15);
  if (tid < kSortwBins) s_dst[tid] = v.hist(k)[(size_t)tid * v.tiles + tile];
  __syncthreads();
  // exclusive scan of the 4096 counts in (digit, thread) order = place in the sorted tile of the thread's first key with that digit
  int c[16], s = 0;
#pragma unroll
  for (int i = 0; i < 16; ++i) s += c[i] = s_cnt[at(16 * tid + i)];
  int run = sortw_block_scan<false>(s, s_w);
  if ((tid & 15) == 0) s_start[tid >> 4] = run;  // where the digit's run starts in the sorted tile
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    s_cnt[at(16 * tid + i)] = run;
    run += c[i];
  }
  __syncthreads();
  unsigned long long seen = 0;
#pragma unroll
  for (int j = 0; j < kSortwPer; ++j)
    if (j < n) {
      const int d = sortw_digit(key[j], pass);
      s_key[s_cnt[at(d * kWThreads + tid)] + (int)((seen >> (kSortwBits * d)) & 15)] = key[j];
      seen += 1ull << (kSortwBits * d);
    }
  __syncthreads();
  const int left = v.E - tile * kSortwTile, valid = left < kSortwTile ? left : kSortwTile;
  unsigned* dst = v.keys(k, src ^ 1);
  for (int q = tid; q < valid; q += kWThreads) {
    const unsigned x = s_key[q];
    const int d = sortw_digit(x, pass);
    dst[s_dst[d] + (q - s_start[d])] = x;
  }
}

}  // namespace uglad
