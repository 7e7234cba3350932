// Inverse and log-determinant beyond the LDS Cholesky (chol.h) where no eigen path can take over a matrix Cholesky refuses: Theta_0 =
// (S + t I)^-1 and the loss's logdet / Theta_L^-1 for D > 256, and for the few large matrices of 128 < D <= 256 whose cell takes the matrix
// iteration (host_route.h, Factor::kLdl).  Blocked, unpivoted A = L D L^T with unit lower triangular L and diagonal D of either sign, so that
// log|det A| = sum log|d_i|, sign(det A) = parity of the negative d_i (torch.logdet's NaN for det < 0 comes from that), and
// A^-1 = W^T D^-1 W with W = L^-1 -- also for an indefinite A, e.g. the Theta_L the reference itself produces at D = 512 with parameters
// trained at D = 25 (10 of 512 eigenvalues negative, tests/golden/cell_d512_b1_L15_trained.npz).  For a positive definite matrix this is
// Cholesky's arithmetic up to where the square roots sit.  A pivot that is zero or NaN leaves NaN in the inverse and the log-determinant.
// The caller polishes the inverse with Newton steps on tile products (launch_ns_inverse).
//
// The matrix, padded to the next multiple of 32 (identity on the padding), lives on three workspace slabs of row stride FD + 1, FD =
// ns_fact_dim(D); the pivots and four accumulators sit wherever the kernel keeps them.  The factorisation is a SCHEDULE of steps
// (ldl_schedule) over nine PHASES (ldl_phase), each written once and walked by two kernels:
//   ns_ldl_kernel        one workgroup of 16 waves per matrix walks the whole schedule, a barrier after every step (the default up to D = 256:
//                        0.35 ms there, less than the launches of the other form cost)
//   ns_ldl_phase_kernel  one launch per step, the tiles of the step dealt out over as many workgroups as it has work for (the default beyond:
//                        D = 1024 is 10.5 ms on one CU; the arithmetic is 1 GFLOP)
// Per tile both run the same products in the same k order with the same epilogues: the same bits.
//
// One barrier (or launch boundary) per step is enough, because
//   * a tile phase writes only the tiles it deals out, one wave each, and reads what earlier steps finished: the panel of block column j reads
//     T_jj and the pivots of its diagonal step, the trailing update the panel's M_ij and L_kj;
//   * WSum of diagonal d writes the tiles of diagonal d of sW and reads sW only on diagonals < d (the diagonal blocks T_jj among them);
//   * WMul reads and overwrites its own tile within one wave, so it needs UGLAD_WAVE_SYNC() and nothing more;
//   * the M_ij the panels parked in sW are dead after their trailing update, before the first tile of W is formed over them.
#pragma once
#include "glad_device.h"

namespace uglad {

// What bounds D on this path is the layout: three slabs of F x (F + 1) floats per matrix, F = ns_fact_dim(D) -- 1024 up to D = 1024 (round
// 3's layout and timings: a row stride of 2049 floats for every D made the factorisation of a 512 x 512 matrix 8 x slower, 17 ms, rows 64
// cache lines apart), 2048 beyond (round 4: D up to 2048).
constexpr int kNsMaxD = 2048;
constexpr int kNsFactSmall = 1024;
__host__ __device__ constexpr int ns_fact_dim(int D) { return D <= kNsFactSmall ? kNsFactSmall : kNsMaxD; }
constexpr int kNsLdlWaves = 16;    // ns_ldl_kernel: operands live in L2, not LDS: a tile product is a round trip of latency, so 16 waves share the tiles
constexpr int kLdlWavesPerWg = 4;  // ns_ldl_phase_kernel

// One 32 x 32 diagonal block by one wave: L_jj (unit lower) -> sL, T = L_jj^-1 -> sW, the pivots -> dv[d0 .. d0 + 31].
template <int LD>
__device__ __forceinline__ bool ldl_diag_block(float* __restrict__ sL, float* __restrict__ sW, float* __restrict__ dv, int d0, float& log2sum,
                                               int& negatives) {
  const int lane = threadIdx.x & 63, r = lane & 31;
  float b[32];
#pragma unroll
  for (int c = 0; c < 32; ++c) b[c] = sL[(d0 + r) * LD + d0 + c];
  bool ok = true;
  float mine = 1.f;
#pragma unroll
  for (int c = 0; c < 32; ++c) {
    const float piv = bcast_lane(b[c], c);  // d_c
    ok = ok && (piv != 0.f) && (piv == piv);
    log2sum += __builtin_amdgcn_logf(fabsf(piv));
    negatives += (piv < 0.f) ? 1 : 0;
    if (r == c) mine = piv;
    const float l = (r == c) ? 1.f : ((r > c) ? b[c] / piv : 0.f);  // column c of L
    // a[r][c2] -= l[r][c] d_c l[c2][c], and d_c l[c2][c] is what lane c2 still holds in b[c]
#pragma unroll
    for (int c2 = c + 1; c2 < 32; ++c2) b[c2] = fmaf(-l, bcast_lane(b[c], c2), b[c2]);
    b[c] = l;
  }
  float t[32];  // T = L^-1 (unit lower), lane = column q
#pragma unroll
  for (int i = 0; i < 32; ++i) {
    float acc = (i == r) ? 1.f : 0.f;
#pragma unroll
    for (int k = 0; k < i; ++k) acc = fmaf(-bcast_lane(b[k], i), t[k], acc);
    t[i] = acc;
  }
  if (lane < 32) {
#pragma unroll
    for (int c = 0; c < 32; ++c) sL[(d0 + r) * LD + d0 + c] = b[c];
#pragma unroll
    for (int i = 0; i < 32; ++i) sW[(d0 + i) * LD + d0 + r] = t[i];
    dv[d0 + r] = mine;
  }
  return ok;
}

// One matrix of a call: its three slabs (row stride LD; sL: the matrix -> L -> D^-1 W, sW: T_jj, M_ij -> W, sX: the result, both triangles),
// dv: DP pivots, acc: four floats -- sum of log2 |pivot|, number of negative pivots, ok flag (1 = fine), one unused --, and what the first and
// the last phase touch: the D x D source, the shift of its diagonal and where the log-determinant goes (may be null).
struct LdlMatrix {
  float *sL, *sW, *sX, *dv, *acc;
  const float* src;
  const float* shift;  // device scalar per group of gs matrices, shift_stride floats apart, or null; read by Init alone, so matrix -> group
  int shift_stride, m, gs;  // (a division, then a dependent load) is left to it: ahead of the switch it would sit in every launch's prologue
  float* logdet_out;
  int D;
};
// Who works on that matrix in this step: this wave among `waves` (tile phases), this thread among `threads` (element phases)
struct LdlTeam {
  int wave, waves, thread, threads;
};

enum { kLdlInit = 0, kLdlDiag, kLdlPanel, kLdlTrail, kLdlWSum, kLdlWMul, kLdlScale, kLdlX, kLdlFinish };

// THE ORDER OF THE PHASES: f(phase, jd, items) for every step of the factorisation of nt x nt tiles; jd: the block column (Diag, Panel, Trail) or
// the diagonal (WSum, WMul); items: tiles (one wave each) or elements (one thread each) of work in the step.  5 nt steps.
template <class F>
__host__ __device__ __forceinline__ void ldl_schedule(int nt, F&& f) {
  const int dp = nt * 32;
  f(kLdlInit, 0, dp * dp);
  for (int j = 0; j < nt; ++j) {
    f(kLdlDiag, j, 1);
    if (j + 1 < nt) {
      f(kLdlPanel, j, nt - 1 - j);
      f(kLdlTrail, j, (nt - 1 - j) * (nt - j) / 2);
    }
  }
  for (int d = 1; d < nt; ++d) {
    f(kLdlWSum, d, nt - d);
    f(kLdlWMul, d, nt - d);
  }
  f(kLdlScale, 0, dp * dp);
  f(kLdlX, 0, nt * (nt + 1) / 2);
  f(kLdlFinish, 0, dp * dp);
}

// One step, by everybody `t` names.  Only the leading nt x nt tiles are touched, nt = ceil(D / 32) (the layout stays that of LD).
template <int LD>
__device__ __forceinline__ void ldl_phase(int phase, int jd, const LdlMatrix& a, const LdlTeam& t) {
  float* const sL = a.sL;
  float* const sW = a.sW;
  float* const sX = a.sX;
  const float* const dv = a.dv;
  const int lane = threadIdx.x & 63, li = lane & 31, D = a.D;
  const int nt = (D + 31) / 32, dp = nt * 32;
  auto store_tile = [&](float* __restrict__ X, int I, int J, const f32x16& acc, float scale) {
#pragma unroll
    for (int e = 0; e < 16; ++e) X[(I * 32 + acc_row(e, lane)) * LD + J * 32 + li] = scale * acc[e];
  };
  f32x16 acc;
  switch (phase) {
    case kLdlInit: {  // the padded matrix -> sL, zeros -> sW, the accumulators
      const float sh = a.shift ? a.shift[(size_t)(a.m / a.gs) * a.shift_stride] : 0.f;
      for (int idx = t.thread; idx < dp * dp; idx += t.threads) {
        const int i = idx / dp, k = idx - i * dp;
        sL[i * LD + k] = (i < D && k < D) ? a.src[(size_t)i * D + k] + ((i == k) ? sh : 0.f) : ((i == k) ? 1.f : 0.f);
        sW[i * LD + k] = 0.f;
      }
      if (t.thread < 4) a.acc[t.thread] = (t.thread == 2) ? 1.f : 0.f;
      break;
    }
    case kLdlDiag: {  // one wave
      if (t.wave != 0) break;
      float l2 = 0.f;
      int neg = 0;
      const bool ok = ldl_diag_block<LD>(sL, sW, a.dv, 32 * jd, l2, neg);
      if (lane == 0) {
        a.acc[0] += l2;
        a.acc[1] += (float)neg;
        if (!ok) a.acc[2] = 0.f;
      }
      break;
    }
    case kLdlPanel: {  // i > j:  M_ij = A_ij T_jj^T (= L_ij D_j) -> sW(i, j);  L_ij = M_ij D_j^-1 -> sL(i, j)
      const int j = jd;
      for (int i = j + 1 + t.wave; i < nt; i += t.waves) {
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] = 0.f;
        mfma_tile(sL + (32 * i) * LD + 32 * j, LD, 1, sW + (32 * j) * LD + 32 * j, 1, LD, 32, acc);
        const float invd = 1.0f / dv[32 * j + li];
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int at = (i * 32 + acc_row(e, lane)) * LD + j * 32 + li;
          sW[at] = acc[e];
          sL[at] = acc[e] * invd;
        }
      }
      break;
    }
    case kLdlTrail: {  // A_ik -= M_ij L_kj^T for j < k <= i
      const int j = jd, nrem = nt - 1 - j, ntile = nrem * (nrem + 1) / 2;
      for (int tl = t.wave; tl < ntile; tl += t.waves) {
        int r = 0, rem = tl;
        while (rem > r) {
          rem -= r + 1;
          ++r;
        }
        const int i = j + 1 + r, k = j + 1 + rem;
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] = 0.f;
        mfma_tile(sW + (32 * i) * LD + 32 * j, LD, 1, sL + (32 * k) * LD + 32 * j, 1, LD, 32, acc);
#pragma unroll
        for (int e = 0; e < 16; ++e) sL[(i * 32 + acc_row(e, lane)) * LD + k * 32 + li] -= acc[e];
      }
      break;
    }
    case kLdlWSum: {  // diagonal d of W = L^-1: sum_{k=j}^{i-1} L_ik W_kj -> sW(i, j), i = j + d
      const int d = jd;
      for (int j = t.wave; j + d < nt; j += t.waves) {
        const int i = j + d;
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] = 0.f;
        for (int k = j; k < i; ++k) mfma_tile(sL + (32 * i) * LD + 32 * k, LD, 1, sW + (32 * k) * LD + 32 * j, LD, 1, 32, acc);
        store_tile(sW, i, j, acc, 1.f);
      }
      break;
    }
    case kLdlWMul: {  // W_ij = -T_ii (that sum)
      const int d = jd;
      for (int j = t.wave; j + d < nt; j += t.waves) {
        const int i = j + d;
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] = 0.f;
        mfma_tile(sW + (32 * i) * LD + 32 * i, LD, 1, sW + (32 * i) * LD + 32 * j, LD, 1, 32, acc);
        UGLAD_WAVE_SYNC();  // (the tile is read by this wave alone and overwritten by it: every lane has its operands)
        store_tile(sW, i, j, acc, -1.f);
      }
      break;
    }
    case kLdlScale: {  // V = D^-1 W (rows scaled) -> sL, lower tiles incl. the diagonal ones (L is dead)
      for (int idx = t.thread; idx < dp * dp; idx += t.threads) {
        const int i = idx / dp, k = idx - i * dp;
        if ((k >> 5) <= (i >> 5)) sL[i * LD + k] = sW[i * LD + k] / dv[i];
      }
      break;
    }
    case kLdlX: {  // X = W^T V on the upper tiles, mirrored -> sX
      const int ntile = nt * (nt + 1) / 2;
      for (int tl = t.wave; tl < ntile; tl += t.waves) {
        int I = 0, J = tl;  // tile tl -> (I <= J) over the nt x nt upper triangle, row by row
        while (J >= nt - I) {
          J -= nt - I;
          ++I;
        }
        J += I;
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] = 0.f;
        for (int k = J; k < nt; ++k) mfma_tile(sW + (32 * k) * LD + 32 * I, 1, LD, sL + (32 * k) * LD + 32 * J, LD, 1, 32, acc);
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int i = I * 32 + acc_row(e, lane), jj = J * 32 + li;
          if (i <= jj) {
            sX[i * LD + jj] = acc[e];
            sX[jj * LD + i] = acc[e];
          }
        }
      }
      break;
    }
    default: {  // kLdlFinish: the log-determinant with torch.logdet's rules; NaN everywhere after a zero / NaN pivot
      const bool ok = a.acc[2] != 0.f;
      const float nan = __builtin_nanf("");
      if (!ok)
        for (int idx = t.thread; idx < dp * dp; idx += t.threads) sX[(idx / dp) * LD + idx % dp] = nan;
      if (t.thread == 0 && a.logdet_out) *a.logdet_out = (!ok || (((int)a.acc[1]) & 1)) ? nan : 0.69314718056f * a.acc[0];
      break;
    }
  }
}

// matrix m of a call: the slabs of its region
template <int FD>
__device__ __forceinline__ LdlMatrix ldl_matrix(int m, const float* __restrict__ src, const float* __restrict__ shift, int shift_stride,
                                                float* __restrict__ slabs, size_t slab_stride, float* __restrict__ logdet_out, int D, int gs) {
  LdlMatrix a;
  a.sL = slabs + (size_t)m * slab_stride;
  a.sW = a.sL + (size_t)FD * (FD + 1);
  a.sX = a.sW + (size_t)FD * (FD + 1);
  a.dv = a.sX + (size_t)FD * (FD + 1);  // the pivots and the accumulators: the head of the region behind the three slabs (the Newton steps'
  a.acc = a.dv + FD;                    // residual, written only after the factorisation: >= D^2 > FD + 4 floats); ns_ldl_kernel keeps them in LDS
  a.src = src + (size_t)m * D * D;
  a.shift = shift;
  a.shift_stride = shift_stride, a.m = m, a.gs = gs;
  a.logdet_out = logdet_out ? logdet_out + m : nullptr;
  a.D = D;
  return a;
}

// X0 = (src + shift I)^-1 -> the third slab, the log-determinant -> logdet_out[m]: one workgroup per matrix walks the schedule; its waves are
// the matrix's waves, its threads the matrix's threads.
template <int FD>
__global__ __launch_bounds__(64 * kNsLdlWaves) void ns_ldl_kernel(const float* __restrict__ src, const float* __restrict__ shift, int shift_stride,
                                                                  float* __restrict__ slabs, size_t slab_stride, float* __restrict__ logdet_out, int D,
                                                                  int gs) {
  __shared__ float s_acc[4];
  __shared__ float s_dv[FD];
  LdlMatrix a = ldl_matrix<FD>(blockIdx.x, src, shift, shift_stride, slabs, slab_stride, logdet_out, D, gs);
  a.dv = s_dv;
  a.acc = s_acc;
  const LdlTeam t{(int)threadIdx.x >> 6, kNsLdlWaves, (int)threadIdx.x, 64 * kNsLdlWaves};
  bool ok = true;
  ldl_schedule((D + 31) / 32, [&](int phase, int jd, int) __attribute__((always_inline)) {
    if (!ok && phase != kLdlFinish) return;  // (uniform) after a zero / NaN pivot: straight to Finish
    ldl_phase<FD + 1>(phase, jd, a, t);
    __syncthreads();
    if (phase == kLdlDiag) ok = s_acc[2] != 0.f;
  });
}

// The same as a sequence of launches, one per step of the schedule (launch_ns_inverse): grid (workgroups of the step, matrices); a launch
// boundary is the barrier.
template <int FD>
__global__ __launch_bounds__(64 * kLdlWavesPerWg) void ns_ldl_phase_kernel(int phase, int jd, const float* __restrict__ src, const float* __restrict__ shift,
                                                                           int shift_stride, float* __restrict__ slabs, size_t slab_stride,
                                                                           float* __restrict__ logdet_out, int D, int gs) {
  const LdlMatrix a = ldl_matrix<FD>(blockIdx.y, src, shift, shift_stride, slabs, slab_stride, logdet_out, D, gs);
  const int tid = threadIdx.x;
  constexpr int kWg = 64 * kLdlWavesPerWg;
  const LdlTeam t{(int)(blockIdx.x * kLdlWavesPerWg) + (tid >> 6), (int)(gridDim.x * kLdlWavesPerWg), (int)(blockIdx.x * kWg) + tid, (int)(gridDim.x * kWg)};
  ldl_phase<FD + 1>(phase, jd, a, t);
}

}  // namespace uglad
