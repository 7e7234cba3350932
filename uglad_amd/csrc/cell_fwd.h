// The forward cell: the LDS-lean kernel (one workgroup per matrix) and, for few large matrices, the launch that finishes its
// eigen-decomposition after the many-workgroup merge of wide_fwd.h.  Templated on NT only: every per-NT unit holds them.
#pragma once
#include "eig_lean.h"

namespace uglad {

// =============================================================================================== cell forward, LDS-lean
// The same cell for D <= 128 on ONE LDS-resident matrix (eig_lean.h): ~75 KB of LDS and <= 128 registers, so two workgroups
// share a CU.  Q holds the eigenvectors, then theta_half, then Z: every hand-over is separated by a barrier.
// Tws: (M, NT, 32, 32) floats of the caller's workspace for the triangular factors of the back-transformation.
// With ONE matrix per group (a direct fit: M = 1) the workgroup is its whole batch, and the step that follows the cell -- the batch mean of
// ||Z - theta_half||^2 and LambdaNN, norm_lambda_kernel -- is done by its thread 0 right behind the norm: one launch and one hand-over less per
// unroll step (round 4: config 1's step is two latency chains and this 5 us kernel).  All null: the separate launch follows as before.
struct LamStep {
  float* nf_sum;       // (G)
  float* lam_next;     // (G)
  float* lam_in_next;  // (G, 2)
  float inv_m;
};
template <int NT>
__global__ __launch_bounds__(kThreads, NT <= 4 ? 4 : 2) void cell_fwd_lean_kernel(const float* __restrict__ S, const float* __restrict__ Zin,
                                                                    const float* __restrict__ lam_ptr,
                                                                    const float* __restrict__ params, float* __restrict__ Zout,
                                                                    float* __restrict__ half_out, float* __restrict__ U_out,
                                                                    float* __restrict__ beta_out,
                                                                    float* __restrict__ normF_partial,
                                                                    float* __restrict__ cond_max,
                                                                    const float* __restrict__ tri, float* __restrict__ Tws,
                                                                    int D, int mode, int gs, int split, LamStep ls) {
  constexpr int DP = NT * 32, LD = DP + 1;
  // the one big matrix: LDS up to D = 128; beyond, the first of the matrix's two workspace slabs (L2-resident) -- the same
  // code then runs on a global pointer, one workgroup per CU
  constexpr bool kGM = DP > 128;
  __shared__ __attribute__((aligned(16))) float sQ_lds[kGM ? 4 : DP * LD];
  float* sQ = kGM ? const_cast<float*>(tri) + (size_t)gridDim.x * kWsPerMatrix<DP> + (size_t)blockIdx.x * big_floats<DP>() : sQ_lds;
  __shared__ __attribute__((aligned(16))) LeanScratch<DP> ws;
  __shared__ float s_phi[DP], s_red[8];
  const size_t base = (size_t)blockIdx.x * D * D;
  const float* Sm = S + base;
  const float* Zm = Zin + base;
  const int grp = blockIdx.x / gs;
  params += (size_t)grp * kNParam;
  const float lam = lam_ptr[grp];
  KSTAMP(16);
#ifdef UGLAD_STAMPS
  const int tid0 = threadIdx.x;
#define tid tid0
  if (tid == 0 && blockIdx.x < 4096) {
    g_cwg[blockIdx.x][0] = __builtin_amdgcn_s_memrealtime();
    unsigned hw, xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    g_cwg[blockIdx.x][2] = ((unsigned long long)xcc << 32) | hw;
  }
  if (tid < 96) ws.stamp[tid] = 0;
  __syncthreads();
  UGLAD_STAMP(ws, 0);
#undef tid
#endif
  if (kGM && split == 2) {
    // few large matrices: stop before the last merge of the divide & conquer; wide_fwd.h carries it out with many workgroups per
    // matrix and cell_fwd_back_kernel picks up from there
    symeig_lean_front<NT>(sQ, D, ws, tri + (size_t)blockIdx.x * 3 * DP, Tws + (size_t)blockIdx.x * NT * 1024);
    return;
  }
  symeig_lean<NT>(sQ, D, ws, tri + (size_t)blockIdx.x * 3 * DP, Zout + base, D, Tws + (size_t)blockIdx.x * NT * 1024);
  KSTAMP(17);
  // (shadow the ones above: nothing derived from the thread index stays live across the eigensolver, whose last merge needs every register)
  const int tid = opaque_v(threadIdx.x), lane = tid & 63, w = tid >> 6;
#ifdef UGLAD_STAMPS
  if (tid < 96 && blockIdx.x < 4) g_lstamps[blockIdx.x][tid] = ws.stamp[tid];
#endif
  // spectrum -> psi(beta) = phi(beta) + alpha beta of the shifted form theta_half = -alpha b + U diag(psi) U^T (glad_device.h)
  float alpha;
  __syncthreads();  // the scratch below aliases the solver's work area (the back-transformation ends with a barrier of its own unless there
                    // are no reflectors, D <= 2)
  {
    const float be = (tid < D) ? ws.d[tid] : 0.f;
    float cond;
    const float ps = shifted_spectrum(be, D, lam, mode, reinterpret_cast<double*>(ws.ds), alpha, cond);  // (the solver's scratch is free)
    if (tid < DP) s_phi[tid] = ps;
    if (cond_max && tid == 0) cond_max[blockIdx.x] = fmaxf(cond_max[blockIdx.x], cond);  // running maximum over the steps of a pass
    if (tid < D && beta_out) beta_out[(size_t)blockIdx.x * D + tid] = be;
  }
  if (U_out) copy_out_matrix(U_out + base, sQ, D, LD);  // the eigenvectors for the backward pass
  __syncthreads();
  KSTAMP(18);
  // U diag(psi) U^T on the upper tiles, psi applied to the A operand on its way into the MFMA
  using T = Tiles<NT, true>;
  f32x16 acc[T::kPerWave];
  {
    const int li = lane & 31, kh = lane >> 5;
#pragma unroll
    for (int nn = 0; nn < T::kPerWave; ++nn) {
      const int t = w + kWaves * nn;
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[nn][e] = 0.f;
      if (t < T::kCount) {
        int I, J;
        T::ij(t, I, J);
        const float* a = sQ + (I * 32 + li) * LD + kh;
        const float* b = sQ + (J * 32 + li) * LD + kh;
        float av[8], bv[8], pv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          av[u] = a[2 * u];
          bv[u] = b[2 * u];
          pv[u] = s_phi[2 * u + kh];
        }
        for (int k0 = 0; k0 < DP; k0 += 16) {
          const int kn = (k0 + 16 < DP) ? k0 + 16 : k0;
          float an[8], bn[8], pn[8];
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            an[u] = a[kn + 2 * u];
            bn[u] = b[kn + 2 * u];
            pn[u] = s_phi[kn + 2 * u + kh];
          }
#pragma unroll
          for (int u = 0; u < 8; ++u) acc[nn] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u] * pv[u], bv[u], acc[nn], 0, 0, 0);
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            av[u] = an[u];
            bv[u] = bn[u];
            pv[u] = pn[u];
          }
        }
      }
    }
  }
  KSTAMP(19);
  // theta_half = -alpha b + (the product), b = S/lam - Z entry by entry with tridiag_kernel's rounding
  if (alpha != 0.f) {
    const float inv_lam = 1.0f / lam;
#pragma unroll
    for (int nn = 0; nn < T::kPerWave; ++nn) {
      const int t = w + kWaves * nn;
      if (t < T::kCount) {
        int I, J;
        T::ij(t, I, J);
        const int j = J * 32 + (lane & 31);
        float sv[16], zv[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int i = I * 32 + acc_row(e, lane);
          const bool in = i <= j && j < D;
          sv[e] = in ? Sm[i * D + j] : 0.f;
          zv[e] = in ? Zm[i * D + j] : 0.f;
        }
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[nn][e] = fmaf(-alpha, fmaf(inv_lam, sv[e], -zv[e]), acc[nn][e]);
      }
    }
  }
  __syncthreads();  // every wave is done reading the eigenvectors
#pragma unroll
  for (int nn = 0; nn < T::kPerWave; ++nn) {  // theta_half, both triangles, into the same buffer
    const int t = w + kWaves * nn;
    if (t < T::kCount) {
      int I, J;
      T::ij(t, I, J);
      const int j = J * 32 + (lane & 31);
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int i = I * 32 + acc_row(e, lane);
        if (i <= j) {
          sQ[i * LD + j] = acc[nn][e];
          sQ[j * LD + i] = acc[nn][e];
        }
      }
    }
  }
  __syncthreads();
  KSTAMP(21);
  if (half_out) {  // (training) theta_half for the backward pass -- before Z overwrites it
    copy_out_matrix(half_out + base, sQ, D, LD);
    __syncthreads();
  }
  // rhoNN + soft threshold on the upper triangle dealt out evenly (rows p and D-1-p together hold D+1 of them): entry e = tid + kThreads q.  An entry
  // is read (from the upper triangle) only by the thread that then overwrites it and its mirror image with Z.
  constexpr int kMaxQ = ((DP / 2) * (DP + 1) + kThreads - 1) / kThreads;
  constexpr int kQ = kMaxQ < 6 ? kMaxQ : 6;
  const int D1 = D + 1, total = ((D + 1) / 2) * D1;
  const int sp = kThreads / D1, sc = kThreads - sp * D1;
  auto entry = [&](int e, int p, int c) -> int {
    if (e >= total) return -1;
    if (c < D - p) return (p << 16) | (p + c);
    const int i = D - 1 - p;
    return (i == p) ? -1 : ((i << 16) | (i + (c - (D - p))));
  };
  float nsum = 0.f;
  {
    int p = tid / D1, c = tid - p * D1;
    for (int q0 = 0; q0 < kMaxQ; q0 += kQ) {
      int pk[kQ];
      float xv[kQ], sv[kQ], zv[kQ], zn[kQ];
#pragma unroll
      for (int u = 0; u < kQ; ++u) {
        pk[u] = (q0 + u < kMaxQ) ? entry(tid + kThreads * (q0 + u), p, c) : -1;
        c += sc;
        p += sp;
        if (c >= D1) {
          c -= D1;
          ++p;
        }
        const int i = pk[u] >> 16, j = pk[u] & 0xffff;
        const bool in = pk[u] >= 0;
        sv[u] = in ? Sm[i * D + j] : 0.f;
        zv[u] = in ? Zm[i * D + j] : 0.f;
        xv[u] = in ? sQ[i * LD + j] : 0.f;
        zn[u] = 0.f;
      }
#pragma unroll
      for (int u = 0; u + 1 < kQ; u += 2) {  // two entries per pass on the packed pipe
        RhoAct2 act;
        rho_forward2(params, (v2f){xv[u], xv[u + 1]}, (v2f){sv[u], sv[u + 1]}, (v2f){zv[u], zv[u + 1]}, act);
        zn[u] = soft_threshold(xv[u], act.rho.x);
        zn[u + 1] = soft_threshold(xv[u + 1], act.rho.y);
      }
      if (kQ & 1) {
        RhoAct act;
        rho_forward(params, xv[kQ - 1], sv[kQ - 1], zv[kQ - 1], act);
        zn[kQ - 1] = soft_threshold(xv[kQ - 1], act.rho);
      }
#pragma unroll
      for (int u = 0; u < kQ; ++u) {
        if (pk[u] >= 0) {
          const int i = pk[u] >> 16, j = pk[u] & 0xffff;
          const float d = zn[u] - xv[u];
          nsum = fmaf((i == j) ? 1.f : 2.f, d * d, nsum);
          sQ[i * LD + j] = zn[u];
          sQ[j * LD + i] = zn[u];
        }
      }
    }
  }
  KSTAMP(22);
  nsum = block_sum(nsum, s_red);  // (its barriers also publish Z)
  if (tid == 0) {
    normF_partial[blockIdx.x] = nsum;
    if (ls.lam_next) {  // (gs = 1: this matrix is its group -- exactly norm_lambda_kernel's thread 0 on a sum of one term)
      ls.nf_sum[grp] = nsum;
      const float nrm = nsum * ls.inv_m;
      ls.lam_in_next[2 * grp] = nrm;
      ls.lam_in_next[2 * grp + 1] = lam;
      ls.lam_next[grp] = lambda_forward(params, nrm, lam);
    }
  }
  copy_out_matrix(Zout + base, sQ, D, LD);
  KSTAMP(20);
#ifdef UGLAD_STAMPS
  if (tid == 0 && blockIdx.x < 4096) g_cwg[blockIdx.x][1] = __builtin_amdgcn_s_memrealtime();
#endif
}

// Few large matrices, third launch of the forward cell's eigen-decomposition: back-transformation of the merged eigenvectors (second
// slab of the matrix), beta and U out for the backward pass.  What follows (theta_half, rhoNN, norm) is wide_gemm_kernel's.
template <int NT>
__global__ __launch_bounds__(kThreads, 2) void cell_fwd_back_kernel(const float* __restrict__ tri, float* __restrict__ Tws,
                                                                    const float* __restrict__ R, float* __restrict__ U_out,
                                                                    float* __restrict__ beta_out, int D, int nm) {
  // grid (workgroups per matrix, matrices): wave w of workgroup blockIdx.x owns the 16-column strip kWaves blockIdx.x + w, kept in LDS
  constexpr int DP = NT * 32, LD = DP + 1;
  __shared__ __attribute__((aligned(16))) LeanScratch<DP> ws;
  __shared__ __attribute__((aligned(16))) float s_strips[kWaves * DP * 16];
  const int m = blockIdx.y, wg = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  float* Q = const_cast<float*>(tri) + (size_t)nm * kWsPerMatrix<DP> + (size_t)m * big_floats<DP>() + big_floats<DP>() / 2;
  const size_t base = (size_t)m * D * D;
  const float* tri_m = tri + (size_t)m * 3 * DP;
#ifdef UGLAD_STAMPS
  if (tid < 96) ws.stamp[tid] = 0;
  __syncthreads();
#endif
  back_transform_lean<NT>(Q, D, ws, R + base, D, tri_m + 2 * DP, Tws + (size_t)m * NT * 1024 + (size_t)wg * NT * 512, s_strips, wg);
  if (wg == 0 && beta_out && tid < D) beta_out[(size_t)m * D + tid] = tri_m[tid];
  const int strip = kWaves * wg + wv, l16 = lane & 15, g = lane >> 4;
  if (16 * strip < DP) {  // the strip back to the slab (theta_half reads it there) and out for the backward pass
    const float* sq = s_strips + (size_t)wv * DP * 16;
    const int col = 16 * strip + l16;
    for (int r0 = 0; r0 < DP; r0 += 4) {
      const int row = r0 + g;
      const float v = sq[row * 16 + l16];
      Q[row * LD + col] = v;
      if (U_out && row < D && col < D) U_out[base + (size_t)row * D + col] = v;
    }
  }
}

}  // namespace uglad
