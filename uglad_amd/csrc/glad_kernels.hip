// libuglad_hip.so -- kernels and C ABI of the unrolled GLAD hot path for gfx950.  See include/uglad_hip.h.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdlib>
#include <cstring>

#include "../../include/uglad_hip.h"
#include "glad_device.h"
#include "eig_dc.h"
#include "eig_lean.h"
#include "tridiag_wave.h"
#include "chol.h"

namespace uglad {

#ifdef UGLAD_STAMPS
__device__ unsigned long long g_cwg[4096][3];     // diagnostic build: per workgroup of the last lean cell_fwd: start, end, hardware id
__device__ unsigned long long g_lstamps[4][96];  // diagnostic build: solver phase stamps of workgroups 0..3 of the last lean cell_fwd
__device__ unsigned long long g_kstamps[32];  // diagnostic build: phase stamps of workgroup 0 of the last cell_fwd / cell_bwd
#define KSTAMP(i) do { if (threadIdx.x == 0 && blockIdx.x == 0) g_kstamps[i] = __builtin_amdgcn_s_memtime(); } while (0)
#elif defined(UGLAD_PHASE_EXIT)
#define KSTAMP(i) do { if (g_exit_at == 100 + (i)) __builtin_amdgcn_endpgm(); } while (0)
#else
#define KSTAMP(i) do {} while (0)
#endif

// Coalesced copy of the D x D matrix in LDS (row stride LD) to global memory: 16 bytes per lane and store where the rows allow it
// (D a multiple of 4 and an aligned destination), else 4.  The tail of such a copy is bound by the number of store
// instructions, not by bytes.
__device__ __forceinline__ void copy_out_matrix(float* __restrict__ dst, const float* __restrict__ src, int D, int LD) {
  const int tid = threadIdx.x;
  if (((D & 3) == 0) && ((reinterpret_cast<size_t>(dst) & 15) == 0)) {
    // (a half wave reads one row as 32 pieces of 16 bytes: stride 4 over the odd row stride, 8 banks hit four times.  Dealt out as
    // 4 rows x 8 pieces the reads are conflict-free, but a half wave's store is then four 128-byte segments instead of 512 contiguous
    // bytes and the forward cell as a whole 1.3 % slower on a same-box A/B: profiles/r03_lean_phase_counters.txt)
    const int D4 = D >> 2;
    for (int idx = tid; idx < D * D4; idx += kThreads) {
      const int i = idx / D4, j = 4 * (idx - i * D4);
      const float* p = src + i * LD + j;
      f4 v = {p[0], p[1], p[2], p[3]};
      *reinterpret_cast<f4*>(dst + (size_t)i * D + j) = v;
    }
  } else {
    const int si = kThreads / D, sj = kThreads - si * D;
    int i = tid / D, j = tid - i * D;
    for (int idx = tid; idx < D * D; idx += kThreads) {
      dst[idx] = src[i * LD + j];
      j += sj;
      i += si;
      if (j >= D) {
        j -= D;
        ++i;
      }
    }
  }
}

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

// =============================================================================================== cell backward
// Replaces autograd through glad.py:139-144, torch_sqrtm.py:32-46, glad_params.py:61-81.
// The rhoNN / threshold backward (the expensive entrywise part) works on the upper triangle dealt out evenly over the threads,
// as in the forward epilogue; the thread that differentiates the threshold at (i,j) keeps the direct term dL/dZ_ij in a
// register and adds (G_B)_ij, which comes back through LDS from the last GEMM, at the very end.  Symmetric products
// (C = U^T G U, G_B) are formed on the 10 upper tiles only; the result leaves through LDS with coalesced stores.
#define UGLAD_CELL_BWD_NAME cell_bwd_kernel
#define UGLAD_CELL_BWD_GS 0
#include "cell_bwd.h"
#undef UGLAD_CELL_BWD_NAME
#undef UGLAD_CELL_BWD_GS
#define UGLAD_CELL_BWD_NAME cell_bwd_gs_kernel
#define UGLAD_CELL_BWD_GS 1
#include "cell_bwd.h"
#undef UGLAD_CELL_BWD_NAME
#undef UGLAD_CELL_BWD_GS

#ifndef UGLAD_TU_NT
}  // namespace uglad
#include "wide_bwd.h"
#include "wide_fwd.h"
#include "wide_ns.h"
namespace uglad {
#endif

// =============================================================================================== Theta_0 and its gradient
// One Newton step on an approximate inverse: X (symmetric, in sA; whatever sits on the padding is ignored) of A = Asrc + shift I ->
// out = X + X (I - A X), computed on the upper tiles and mirrored.  sV is scratch.  Takes X from the ~1e-6 of a spectral or Cholesky
// inverse in fp32 to the ~1e-7 of the LU-based inverse the reference calls.
template <int NT>
__device__ __forceinline__ void newton_inverse_to_global(float* __restrict__ sA, float* __restrict__ sV, float* __restrict__ out, int D,
                                                         const float* __restrict__ Asrc, float shift) {
  constexpr int DP = NT * 32, LD = DP + 1;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  using T = Tiles<NT, true>;
  f32x16 acc[T::kPerWave];
  for (int idx = tid; idx < DP * DP; idx += kThreads) {
    const int i = idx / DP, k = idx - i * DP;
    sV[i * LD + k] = (i < D && k < D) ? Asrc[i * D + k] + ((i == k) ? shift : 0.f) : 0.f;
  }
  __syncthreads();
  {  // R = I - A X (all tiles) -> sV
    using TF = Tiles<NT, false>;
    f32x16 accf[TF::kPerWave];
    gemm_lds<NT, false, false, false>(sV, sA, accf);
    __syncthreads();
#pragma unroll
    for (int n = 0; n < TF::kPerWave; ++n) {
      const int t = w + kWaves * n;
      if (t < TF::kCount) {
        int I, J;
        TF::ij(t, I, J);
        const int j = J * 32 + (lane & 31);
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int i = I * 32 + acc_row(e, lane);
          sV[i * LD + j] = ((i == j && i < D) ? 1.f : 0.f) - accf[n][e];
        }
      }
    }
  }
  __syncthreads();
  gemm_lds<NT, false, false, true>(sA, sV, acc);  // X R on the upper tiles
#pragma unroll
  for (int n = 0; n < T::kPerWave; ++n) {
    const int t = w + kWaves * n;
    if (t < T::kCount) {
      int I, J;
      T::ij(t, I, J);
      const int j = J * 32 + (lane & 31);
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int i = I * 32 + acc_row(e, lane);
        if (i <= j && j < D) {
          const float v = sA[i * LD + j] + acc[n][e];
          out[i * D + j] = v;
          if (i != j) out[j * D + i] = v;
        }
      }
    }
  }
}


// f(A) = V diag(f) V^T of the symmetric matrix whose eigenvectors sit in sV (stride DP+1) -> out (D x D, global), computed on
// the upper 32x32 tiles and mirrored so the result is exactly symmetric.  sA is scratch (DP x (DP+1)).
// With Asrc != nullptr, f = 1/(eigenvalue) and the result X ~ (Asrc + shift I)^-1 gets one Newton step X <- X + X (I - A X)
// before it is stored: the eigenvectors of an fp32 solver are orthogonal to ~1e-6 (LAPACK's ssyevd is no better), which is
// the accuracy of V diag(f) V^T, while the step leaves the ~1e-7 of an LU-based inverse (what the reference calls).  That
// matters for the gradients: dL/dTheta_L = -Theta^-1 + S is a small difference of two O(1) matrices near the optimum.
template <int NT>
__device__ __forceinline__ void spectral_to_global(float* __restrict__ sA, float* __restrict__ sV,
                                                   const float* __restrict__ s_f, float* __restrict__ out, int D,
                                                   const float* __restrict__ Asrc = nullptr, float shift = 0.f) {
  constexpr int DP = NT * 32, LD = DP + 1;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  for (int idx = tid; idx < DP * DP; idx += kThreads) {
    const int i = idx / DP, k = idx - i * DP;
    sA[i * LD + k] = sV[i * LD + k] * s_f[k];
  }
  __syncthreads();
  using T = Tiles<NT, true>;
  f32x16 acc[T::kPerWave];
  gemm_lds<NT, false, true, true>(sA, sV, acc);
  if (Asrc == nullptr) {
#pragma unroll
    for (int n = 0; n < T::kPerWave; ++n) {
      const int t = w + kWaves * n;
      if (t < T::kCount) {
        int I, J;
        T::ij(t, I, J);
        const int j = J * 32 + (lane & 31);
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int i = I * 32 + acc_row(e, lane);
          if (i <= j && j < D) {
            out[i * D + j] = acc[n][e];
            if (i != j) out[j * D + i] = acc[n][e];
          }
        }
      }
    }
    return;
  }
  __syncthreads();  // every wave is done reading sA / sV
  // X (symmetric, zero on the padding) -> sA ; A = Asrc + shift I -> sV
#pragma unroll
  for (int n = 0; n < T::kPerWave; ++n) {
    const int t = w + kWaves * n;
    if (t < T::kCount) {
      int I, J;
      T::ij(t, I, J);
      const int j = J * 32 + (lane & 31);
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int i = I * 32 + acc_row(e, lane);
        if (i <= j) {
          sA[i * LD + j] = acc[n][e];
          sA[j * LD + i] = acc[n][e];
        }
      }
    }
  }
  newton_inverse_to_global<NT>(sA, sV, out, D, Asrc, shift);
}

// Theta_0 = (S + t I)^-1 through the eigendecomposition of S (the same in-LDS solver as the cell): V diag(1/(s_i + t)) V^T.
template <int NT>
__global__ __launch_bounds__(kThreads) void init_inverse_kernel(const float* __restrict__ S,
                                                                const float* __restrict__ params,
                                                                float* __restrict__ theta0,
                                                                float* __restrict__ tri, int D, int gs,
                                                                const int* __restrict__ only_flagged) {
  constexpr int DP = NT * 32, LD = DP + 1;
  UGLAD_BIG_BUFFERS(sA, eig_buf0_floats<DP>(), sV, DP * LD, tri)
  __shared__ __attribute__((aligned(16))) EigScratch<DP> ws;
  __shared__ float s_f[DP];
  if (only_flagged && only_flagged[blockIdx.x] == 0) return;  // (the Cholesky kernel has done this matrix)
  const int tid = threadIdx.x;
  const size_t base = (size_t)blockIdx.x * D * D;
  const float t = params[(size_t)(blockIdx.x / gs) * kNParam + P_T];
  symeig_from_tridiagonal<NT>(sA, sV, D, ws, tri + (size_t)blockIdx.x * 3 * DP, theta0 + base, D);
  if (tid < DP) s_f[tid] = (tid < D) ? 1.0f / (ws.d[tid] + t) : 0.f;
  __syncthreads();
  spectral_to_global<NT>(sA, sV, s_f, theta0 + base, D, S + base, t);
}

constexpr float kCholNewtonRatio = 100.f;  // max / min Cholesky pivot beyond which the matrix goes to the eigen path and its Newton step
// ---- the same two results by blocked Cholesky (chol.h), D <= 128: Theta_0 = (S + t I)^-1 ...
// flags[m] = 0: done; 1: a pivot was not > 0 (S + t I is not positive definite, or holds a NaN): the eigen path recomputes this matrix.
// (lower tiles of the DP x DP matrix: element idx of the packed storage -> (i, j); 32 consecutive idx = one row of a tile)
template <int NT>
__device__ __forceinline__ void chol_packed_coords(int idx, int& i, int& j) {
  const int t = idx >> 10, r = (idx >> 5) & 31, c = idx & 31;
  int I = 0, rem = t;
  while (rem > I) {  // slot t = I (I + 1) / 2 + J
    rem -= I + 1;
    ++I;
  }
  i = 32 * I + r;
  j = 32 * rem + c;
}

template <int NT>
__global__ __launch_bounds__(kThreads, 4) void chol_init_kernel(const float* __restrict__ S, const float* __restrict__ params,
                                                             float* __restrict__ theta0, int* __restrict__ flags, int D, int gs) {
  __shared__ __attribute__((aligned(16))) float sP[chol_lower_tiles(NT) * kTF];
  __shared__ __attribute__((aligned(16))) float sQ[(NT > 1 ? chol_offdiag_tiles(NT) : 1) * kTF];
  __shared__ int s_flag;
  __shared__ float s_log[3];
  const int tid = threadIdx.x;
  const size_t base = (size_t)blockIdx.x * D * D;
  const float t = params[(size_t)(blockIdx.x / gs) * kNParam + P_T];
  // the lower tiles of S + t I (identity on the padding); eight loads in flight per thread, from clamped addresses
  constexpr int kElems = chol_lower_tiles(NT) * 1024;
  for (int idx0 = 0; idx0 < kElems; idx0 += 8 * kThreads) {
    float v[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int idx = idx0 + q * kThreads + tid;
      int i, k;
      chol_packed_coords<NT>(idx < kElems ? idx : 0, i, k);
      const bool in = i < D && k < D;
      const float x = S[base + (in ? i * D + k : 0)];
      v[q] = in ? x + ((i == k) ? t : 0.f) : ((i == k) ? 1.f : 0.f);
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int idx = idx0 + q * kThreads + tid;
      if (idx < kElems) sP[(idx >> 10) * kTF + ((idx >> 5) & 31) * kTS + (idx & 31)] = v[q];
    }
  }
  __syncthreads();
  float logdet, pivot_ratio;
  bool ok = chol_inverse_packed<NT>(sP, sQ, logdet, pivot_ratio, &s_flag, s_log);
  // W^T W from a Cholesky factor is at the ~2e-7 of an LU inverse while the matrix is well conditioned (uGLAD's inputs: cond 10 ... 50).
  // Its error grows with the condition number: a matrix whose pivots spread by more than kCholNewtonRatio goes to the eigen path like one
  // that is not positive definite -- that path ends with a Newton step (Theta within 1.7e-5 instead of 2.8e-5 of fp64 at cond(S + tI) 3500).
  ok = ok && !(pivot_ratio > kCholNewtonRatio);
  if (tid == 0) flags[blockIdx.x] = ok ? 0 : 1;
  if (!ok) return;
  float* __restrict__ out = theta0 + base;
  for (int idx = tid; idx < D * D; idx += kThreads) {
    const int i = idx / D, j = idx - i * D;
    out[idx] = chol_packed_at(sP, i, j);
  }
}

#ifndef UGLAD_TU_NT
__global__ void init_diag_kernel(const float* __restrict__ S, const float* __restrict__ params,
                                 float* __restrict__ theta0, int D, size_t total, int gs) {
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
    const size_t m = idx / ((size_t)D * D);
    const float t = params[(m / gs) * kNParam + P_T];
    const int r = (int)(idx - m * (size_t)D * D);
    const int i = r / D, j = r - i * D;
    theta0[idx] = (i == j) ? 1.0f / (S[idx] + t) : 0.f;
  }
}
#endif

// gt_partial[m] = -<sym(G0), Theta0^2>
template <int NT>
__global__ __launch_bounds__(kThreads) void init_bwd_kernel(const float* __restrict__ theta0,
                                                            const float* __restrict__ G0, float* __restrict__ gt_partial,
                                                            float* __restrict__ gws, int D) {
  constexpr int DP = NT * 32, LD = DP + 1;
  UGLAD_BIG_BUFFERS(sX, DP * LD, sUnused, 4, gws)
  __shared__ float s_red[8];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const size_t base = (size_t)blockIdx.x * D * D;
  for (int idx0 = 0; idx0 < DP * DP; idx0 += 8 * kThreads) {  // eight loads in flight per thread (clamped addresses)
    float v[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int idx = idx0 + q * kThreads + tid;
      const int i = idx / DP, k = idx - i * DP;
      const bool in = (idx < DP * DP) && i < D && k < D;
      const float x = theta0[base + (in ? i * D + k : 0)];
      v[q] = in ? x : 0.f;
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int idx = idx0 + q * kThreads + tid;
      if (idx < DP * DP) sX[(idx / DP) * LD + (idx % DP)] = v[q];
    }
  }
  __syncthreads();
  using T = Tiles<NT, false>;
  f32x16 acc[T::kPerWave];
  gemm_lds<NT, false, false, false>(sX, sX, acc);
  float sum = 0.f;
#pragma unroll
  for (int n = 0; n < T::kPerWave; ++n) {
    const int t = w + kWaves * n;
    if (t < T::kCount) {
      int I, J;
      T::ij(t, I, J);
      const int j = J * 32 + (lane & 31);
#pragma unroll
      for (int e = 0; e < 16; ++e) {  // (unconditional loads from clamped addresses: all sixteen in flight)
        const int i = I * 32 + acc_row(e, lane);
        const bool in = i < D && j < D;
        const float gv = G0[base + (in ? j * D + i : 0)];
        sum = fmaf(in ? gv : 0.f, acc[n][e], sum);  // <G0, (Theta0^2)^T>
      }
    }
  }
  sum = block_sum(sum, s_red);
  if (tid == 0) gt_partial[blockIdx.x] = -sum;
}

// Theta_0 = (S + t I)^-1 with respect to S:  gS -= Theta0 sym(G0) Theta0.  T = Theta0 G0 on all tiles, then T Theta0 on the upper tiles,
// subtracted from gS_ij and mirrored into gS_ji (exactly symmetric).  The 42 parameter gradients stay with init_bwd_kernel.
template <int NT>
__global__ __launch_bounds__(kThreads) void init_bwd_gs_kernel(const float* __restrict__ theta0, const float* __restrict__ G0,
                                                               float* __restrict__ gS, float* __restrict__ gws, int D) {
  constexpr int DP = NT * 32, LD = DP + 1;
  UGLAD_BIG_BUFFERS(sX, DP * LD, sY, DP * LD, gws)
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const size_t base = (size_t)blockIdx.x * D * D;
  for (int idx = tid; idx < DP * DP; idx += kThreads) {
    const int i = idx / DP, k = idx - i * DP;
    const bool in = i < D && k < D;
    sX[i * LD + k] = in ? theta0[base + i * D + k] : 0.f;
    sY[i * LD + k] = in ? 0.5f * (G0[base + i * D + k] + G0[base + k * D + i]) : 0.f;
  }
  __syncthreads();
  {
    f32x16 acc[Tiles<NT, false>::kPerWave];
    gemm_lds<NT, false, false, false>(sX, sY, acc);
    __syncthreads();
    store_tiles<NT>(sY, acc);
  }
  __syncthreads();
  using T = Tiles<NT, true>;
  f32x16 acc[T::kPerWave];
  gemm_lds<NT, false, false, true>(sY, sX, acc);
#pragma unroll
  for (int n = 0; n < T::kPerWave; ++n) {
    const int t = w + kWaves * n;
    if (t < T::kCount) {
      int I, J;
      T::ij(t, I, J);
      const int j = J * 32 + (lane & 31);
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int i = I * 32 + acc_row(e, lane);
        if (i <= j && j < D) {
          const float v = gS[base + i * D + j] - acc[n][e];
          gS[base + i * D + j] = v;
          if (i != j) gS[base + j * D + i] = v;
        }
      }
    }
  }
}

#ifndef UGLAD_TU_NT
// Theta_0 = diag(1 / (S_ii + t)) with respect to S:  gS_ii -= G0_ii Theta0_ii^2.  One thread per diagonal entry.
__global__ void init_bwd_diag_gs_kernel(const float* __restrict__ theta0, const float* __restrict__ G0, float* __restrict__ gS, int D,
                                        size_t total) {
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
    const size_t m = idx / D;
    const size_t at = m * D * D + (idx - m * D) * (D + 1);
    const float d = theta0[at];
    gS[at] -= G0[at] * d * d;
  }
}
#endif

#ifndef UGLAD_TU_NT
__global__ __launch_bounds__(kThreads) void init_bwd_diag_kernel(const float* __restrict__ theta0,
                                                                 const float* __restrict__ G0,
                                                                 float* __restrict__ gt_partial, int D) {
  __shared__ float s_red[8];
  const size_t base = (size_t)blockIdx.x * D * D;
  float sum = 0.f;
  for (int i = threadIdx.x; i < D; i += kThreads) {
    const float d = theta0[base + i * D + i];
    sum = fmaf(G0[base + i * D + i], d * d, sum);
  }
  sum = block_sum(sum, s_red);
  if (threadIdx.x == 0) gt_partial[blockIdx.x] = -sum;
}
#endif

// =============================================================================================== loss
__device__ __forceinline__ float log_cosh(float x) {
  const float a = fabsf(x);
  return a + log1pf(expf(-2.f * a)) - 0.69314718056f;
}

// loss partial + Theta^-1 through the eigendecomposition Theta = V diag(beta) V^T:  logdet = sum log|beta_i| with the sign of
// prod beta_i deciding NaN (det < 0) / -inf (det = 0) as torch.logdet does; Theta^-1 = V diag(1/beta) V^T.
template <int NT>
__global__ __launch_bounds__(kThreads) void loss_fwd_kernel(const float* __restrict__ theta, const float* __restrict__ S,
                                                            int s_batch, const float* __restrict__ struct_theta,
                                                            float* __restrict__ loss_partial,
                                                            float* __restrict__ theta_inv,
                                                            float* __restrict__ tri, int D, const int* __restrict__ only_flagged) {
  constexpr int DP = NT * 32, LD = DP + 1;
  UGLAD_BIG_BUFFERS(sA, eig_buf0_floats<DP>(), sV, DP * LD, tri)
  __shared__ __attribute__((aligned(16))) EigScratch<DP> ws;
  __shared__ float s_f[DP], s_red[8];
  if (only_flagged && only_flagged[blockIdx.x] == 0) return;  // (the Cholesky kernel has done this matrix)
  const int tid = threadIdx.x;
  const size_t base = (size_t)blockIdx.x * D * D;
  const size_t sbase = (size_t)(blockIdx.x % s_batch) * D * D;
  float tr = 0.f;
  for (int idx = tid; idx < D * D; idx += kThreads) {
    const int i = idx / D, j = idx - i * D;
    const float th = theta[base + idx];
    tr = fmaf(S[sbase + j * D + i], th, tr);
    if (struct_theta) {
      const float mask = (1.f - struct_theta[sbase + idx]) - ((i == j) ? 1.f : 0.f);
      tr += log_cosh(th * mask);
    }
  }
  tr = block_sum(tr, s_red);
  symeig_from_tridiagonal<NT>(sA, sV, D, ws, tri + (size_t)blockIdx.x * 3 * DP, theta_inv + base, D);
  float lad = 0.f, neg = 0.f, zero = 0.f;
  if (tid < DP) {
    float f = 0.f;
    if (tid < D) {
      const float be = ws.d[tid];
      f = 1.0f / be;
      lad = logf(fabsf(be));
      neg = (be < 0.f) ? 1.f : 0.f;
      zero = (be == 0.f) ? 1.f : 0.f;
    }
    s_f[tid] = f;
  }
  lad = block_sum(lad, s_red);
  neg = block_sum(neg, s_red);
  zero = block_sum(zero, s_red);
  spectral_to_global<NT>(sA, sV, s_f, theta_inv + base, D, theta + base, 0.f);
  if (tid == 0) {
    float logdet = lad;
    if (((int)neg) & 1) logdet = __builtin_nanf("");
    if (zero > 0.f) logdet = -__builtin_inff();
    loss_partial[blockIdx.x] = -logdet + tr;
  }
}

// ... and the loss partial -logdet(Theta) + tr(S Theta) (+ structure penalty) with Theta^-1 for the backward pass (loss_fwd_kernel's outputs)
template <int NT>
__global__ __launch_bounds__(kThreads, 4) void chol_loss_kernel(const float* __restrict__ theta, const float* __restrict__ S, int s_batch,
                                                             const float* __restrict__ struct_theta, float* __restrict__ loss_partial,
                                                             float* __restrict__ theta_inv, int* __restrict__ flags, int D) {
  __shared__ __attribute__((aligned(16))) float sP[chol_lower_tiles(NT) * kTF];
  __shared__ __attribute__((aligned(16))) float sQ[(chol_offdiag_tiles(NT) > kWaves ? chol_offdiag_tiles(NT) : kWaves) * kTF];  // (>= one tile per wave)
  __shared__ int s_flag;
  __shared__ float s_log[3], s_red[8];
  const int tid = threadIdx.x;
  const size_t base = (size_t)blockIdx.x * D * D;
  const size_t sbase = (size_t)(blockIdx.x % s_batch) * D * D;
  float tr = 0.f;
  constexpr int kElems = chol_lower_tiles(NT) * 1024;
  for (int idx = tid; idx < kElems; idx += kThreads) {  // identity on the padding (LDS only)
    int i, k;
    chol_packed_coords<NT>(idx, i, k);
    if (i >= D || k >= D) sP[(idx >> 10) * kTF + ((idx >> 5) & 31) * kTS + (idx & 31)] = (i == k) ? 1.f : 0.f;
  }
  // The trace term sum_ij S_ij Theta_ji and the lower tiles of Theta -> LDS from ONE pass over Theta, tile by tile: a wave takes the pair
  // (S_IJ, Theta_JI), both read along their rows (128 contiguous bytes per half wave), and transposes S_IJ through a tile of LDS -- read
  // straight from memory the transposed operand costs a cache line per element (the kernel took 270 us against Theta_0's 160).
  {
    const int lane = tid & 63, w = tid >> 6, c = lane & 31, rh = lane >> 5;
    float* __restrict__ sT = sQ + w * kTF;  // one scratch tile per wave (sQ is idle until W = L^-1)
    for (int t = w; t < NT * NT; t += kWaves) {
      const int I = t / NT, J = t - I * NT;
      float sv[16], th[16];
#pragma unroll
      for (int it = 0; it < 16; ++it) {  // rows 2 it + rh of both tiles, column c: 32 loads in flight per lane
        const int r = 2 * it + rh;
        const int si = 32 * I + r, sj = 32 * J + c;  // S_IJ[r][c]
        const int ti = 32 * J + r, tj = 32 * I + c;  // Theta_JI[r][c]
        const float xs = S[sbase + ((si < D && sj < D) ? si * D + sj : 0)];
        const float xt = theta[base + ((ti < D && tj < D) ? ti * D + tj : 0)];
        sv[it] = (si < D && sj < D) ? xs : 0.f;
        th[it] = (ti < D && tj < D) ? xt : 0.f;
      }
      UGLAD_WAVE_SYNC();  // (the wave's previous tile has been read by all its lanes)
#pragma unroll
      for (int it = 0; it < 16; ++it) sT[(2 * it + rh) * kTS + c] = sv[it];
      UGLAD_WAVE_SYNC();  // a wave's own LDS writes are visible to its own later reads; other waves use other tiles
#pragma unroll
      for (int it = 0; it < 16; ++it) {
        const int r = 2 * it + rh;
        const int ti = 32 * J + r, tj = 32 * I + c;
        if (ti < D && tj < D) {
          tr = fmaf(sT[c * kTS + r], th[it], tr);  // S_IJ[c][r] Theta_JI[r][c]
          if (struct_theta) {
            const float mask = (1.f - struct_theta[sbase + (size_t)ti * D + tj]) - ((ti == tj) ? 1.f : 0.f);
            tr += log_cosh(th[it] * mask);
          }
          if (J >= I) sP[chol_slot(J, I) * kTF + r * kTS + c] = th[it];
        }
      }
    }
  }
  tr = block_sum(tr, s_red);
  __syncthreads();
  float logdet, pivot_ratio;
  bool ok = chol_inverse_packed<NT>(sP, sQ, logdet, pivot_ratio, &s_flag, s_log);
  ok = ok && !(pivot_ratio > kCholNewtonRatio);  // (ill-conditioned: the eigen path with its Newton step, as for Theta_0)
  if (tid == 0) flags[blockIdx.x] = ok ? 0 : 1;
  if (!ok) return;
  if (tid == 0) loss_partial[blockIdx.x] = -logdet + tr;
  float* __restrict__ out = theta_inv + base;
  for (int idx = tid; idx < D * D; idx += kThreads) {
    const int i = idx / D, j = idx - i * D;
    out[idx] = chol_packed_at(sP, i, j);
  }
}

#ifndef UGLAD_TU_NT
__global__ void loss_bwd_kernel(const float* __restrict__ theta, const float* __restrict__ theta_inv,
                                const float* __restrict__ S, int s_batch, const float* __restrict__ struct_theta,
                                const float* __restrict__ g_up, float scale, float* __restrict__ Gout, int D,
                                size_t total) {
  const float gs = g_up[0] * scale;
  const size_t dd = (size_t)D * D;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
    const size_t m = idx / dd;
    const int r = (int)(idx - m * dd);
    const int i = r / D, j = r - i * D;
    const size_t sb = (m % s_batch) * dd;
    // Theta^-1 (mirrored by loss_fwd) and S are symmetric: read them in place, coalesced, instead of transposed
    float v = -theta_inv[idx] + S[sb + r];
    if (struct_theta) {
      const float mask = (1.f - struct_theta[sb + r]) - ((i == j) ? 1.f : 0.f);
      v += tanhf(theta[idx] * mask) * mask;
    }
    Gout[idx] = gs * v;
  }
}

// dL/dS of the loss, symmetric part: gS_b = g_up[0] * scale * sum over the matrices m that read S_b of (Theta_m + Theta_m^T) / 2
// (one S broadcast against all M matrices when s_batch = 1).  Overwrites gS (s_batch, D, D); a fixed order of the sum over m.
__global__ void loss_bwd_gs_kernel(const float* __restrict__ theta, const float* __restrict__ g_up, float scale, float* __restrict__ gS,
                                   int s_batch, int M, int D) {
  const float gs = g_up[0] * scale * 0.5f;
  const size_t dd = (size_t)D * D, total = (size_t)s_batch * dd;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
    const size_t sb = idx / dd;
    const int r = (int)(idx - sb * dd);
    const int i = r / D, j = r - i * D;
    float v = 0.f;
    for (size_t m = sb; m < (size_t)M; m += s_batch) v += theta[m * dd + i * D + j] + theta[m * dd + j * D + i];
    gS[idx] = gs * v;
  }
}

// dL/dS of one step on the paths whose kernels have no dL/dS variant (the many-workgroups backward, csrc/wide_bwd.h, and the matrix
// iteration, csrc/wide_ns.h), behind their unchanged launches: per upper-triangle entry (i, j) the rhoNN / threshold backward of the step
// is evaluated again from G_next, theta_half, S and Z_in -- the S-feature term, and the Z_in-feature term gz that the step's G_out holds
// together with -G_B (G_out = gz - G_B) -- and gS_ij += (gz - sym(G_out))_ij / lam_k + the S-feature term, mirrored into gS_ji.
__global__ __launch_bounds__(256) void cell_gs_step_kernel(const float* __restrict__ Gnext, const float* __restrict__ S,
                                                           const float* __restrict__ Zin, const float* __restrict__ half,
                                                           const float* __restrict__ lam_ptr, const float* __restrict__ params,
                                                           const float* __restrict__ Gout, float* __restrict__ gS, int D, int gs,
                                                           size_t total) {
  const size_t dd = (size_t)D * D;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
    const size_t m = idx / dd;
    const int r = (int)(idx - m * dd);
    const int i = r / D, j = r - i * D;
    if (j < i) continue;
    const size_t ij = m * dd + r, ji = m * dd + (size_t)j * D + i;
    const int grp = (int)(m / gs);
    const float* p = params + (size_t)grp * kNParam;
    const float lam = lam_ptr[grp];
    const float gn = (i == j) ? Gnext[ij] : 0.5f * (Gnext[ij] + Gnext[ji]);
    const float x = half[ij];
    RhoAct act;
    rho_forward(p, x, S[ij], Zin[ij], act);
    const bool active = fabsf(x) > act.rho;
    const float sgn = (x > 0.f) ? 1.f : ((x < 0.f) ? -1.f : 0.f);
    const float g_rho = active ? -sgn * gn : 0.f;
    const float gz = rho_backward_col(p, act, g_rho, 2);
    const float go = (i == j) ? Gout[ij] : 0.5f * (Gout[ij] + Gout[ji]);
    const float v = gS[ij] + (gz - go) / lam + rho_backward_col(p, act, g_rho, 1);
    gS[ij] = v;
    gS[ji] = v;
  }
}

// C_m = A_m B_m for M matrices of D x D (fp32; 64 x 64 output tile per workgroup, 4 x 4 per thread, k in chunks of 16 through LDS): the
// Theta_0 term of dL/dS beyond the one-workgroup kernels' size.
__global__ __launch_bounds__(256) void gs_gemm_kernel(const float* __restrict__ A, const float* __restrict__ B, float* __restrict__ C, int D) {
  __shared__ float sA[16][65], sB[16][65];
  const size_t base = (size_t)blockIdx.z * D * D;
  const int i0 = blockIdx.y * 64, j0 = blockIdx.x * 64;
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  float acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = 0.f;
  for (int k0 = 0; k0 < D; k0 += 16) {
    for (int e = threadIdx.x; e < 1024; e += 256) {
      const int ar = e >> 4, ac = e & 15, gi = i0 + ar, gk = k0 + ac;
      sA[ac][ar] = (gi < D && gk < D) ? A[base + (size_t)gi * D + gk] : 0.f;
      const int br = e >> 6, bc = e & 63, bk = k0 + br, bj = j0 + bc;
      sB[br][bc] = (bk < D && bj < D) ? B[base + (size_t)bk * D + bj] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      float a[4], b[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        a[q] = sA[k][4 * ty + q];
        b[q] = sB[k][4 * tx + q];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) acc[u][v] = fmaf(a[u], b[v], acc[u][v]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int i = i0 + 4 * ty + u;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int j = j0 + 4 * tx + v;
      if (i < D && j < D) C[base + (size_t)i * D + j] = acc[u][v];
    }
  }
}

// gS -= (R + R^T) / 2, elementwise over M matrices (exactly symmetric when gS is)
__global__ void gs_sub_sym_kernel(const float* __restrict__ R, float* __restrict__ gS, int D, size_t total) {
  const size_t dd = (size_t)D * D;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
    const size_t m = idx / dd;
    const int r = (int)(idx - m * dd);
    const int i = r / D, j = r - i * D;
    gS[idx] -= 0.5f * (R[idx] + R[m * dd + (size_t)j * D + i]);
  }
}
#endif

// =============================================================================================== lambda / reductions
// one thread per group g < G: lam (.., G), lam_in (.., G, 2), params (G, 42)
#ifndef UGLAD_TU_NT
__global__ void lambda_init_kernel(const float* __restrict__ params, float lambda_init, float* __restrict__ lam_out,
                                   float* __restrict__ lam_in, int G) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g < G) {
    lam_in[2 * g] = lambda_init;
    lam_in[2 * g + 1] = 0.f;
    lam_out[g] = lambda_forward(params + (size_t)g * kNParam, lambda_init, 0.f);
  }
}
#endif

#ifndef UGLAD_TU_NT
__global__ void lambda_step_kernel(const float* __restrict__ normF_sum, float inv_M, const float* __restrict__ lam_prev,
                                   const float* __restrict__ params, float* __restrict__ lam_next,
                                   float* __restrict__ lam_in_next, int G) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g < G) {
    const float n = normF_sum[g] * inv_M, lp = lam_prev[g];
    lam_in_next[2 * g] = n;
    lam_in_next[2 * g + 1] = lp;
    lam_next[g] = lambda_forward(params + (size_t)g * kNParam, n, lp);
  }
}
#endif

// sum_partials + lambda_step in one launch (the single-process pass: nothing to exchange between the two).  One block per
// group; same summation order as sum_partials_kernel, so the sharded and the fused path see the same bits per rank.
#ifndef UGLAD_TU_NT
__global__ __launch_bounds__(kThreads) void norm_lambda_kernel(const float* __restrict__ partials, int n, float inv_M,
                                                               const float* __restrict__ lam_prev,
                                                               const float* __restrict__ params, float* __restrict__ nf_sum,
                                                               float* __restrict__ lam_next, float* __restrict__ lam_in_next) {
  __shared__ float s_red[8];
  const int g = blockIdx.x;
  partials += (size_t)g * n;
  float v = 0.f;
  for (int i = threadIdx.x; i < n; i += kThreads) v += partials[i];
  v = block_sum(v, s_red);
  if (threadIdx.x == 0) {
    nf_sum[g] = v;
    const float nrm = v * inv_M, lp = lam_prev[g];
    lam_in_next[2 * g] = nrm;
    lam_in_next[2 * g + 1] = lp;
    lam_next[g] = lambda_forward(params + (size_t)g * kNParam, nrm, lp);
  }
}
#endif

#ifndef UGLAD_TU_NT
__global__ void zero_kernel(float* __restrict__ p, size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) p[i] = 0.f;
}
#endif

// deterministic: fixed per-thread strides, fixed tree
#ifndef UGLAD_TU_NT
__global__ __launch_bounds__(kThreads) void sum_partials_kernel(const float* __restrict__ partials, int n,
                                                                float* __restrict__ out) {
  __shared__ float s_red[8];
  partials += (size_t)blockIdx.x * n;  // one block per group
  float v = 0.f;
  for (int i = threadIdx.x; i < n; i += kThreads) v += partials[i];
  v = block_sum(v, s_red);
  if (threadIdx.x == 0) out[blockIdx.x] = v;
}
#endif

// grad[0] <- sum gt ; grad[1..28] <- column sums of grad_rho_partial ; grad[29..41] <- LambdaNN chain
#ifndef UGLAD_TU_NT
__global__ __launch_bounds__(kThreads) void finish_grads_kernel(const float* __restrict__ gt_partial,
                                                                const float* __restrict__ grad_rho_partial,
                                                                const float* __restrict__ glam_partial,
                                                                const float* __restrict__ lam_in,
                                                                const float* __restrict__ p, float* __restrict__ grad,
                                                                int L, int Mtot, int gs) {
  // one block per group g: matrices [g gs, (g + 1) gs) of the Mtot in the batch; p, grad: (G, 42); lam_in: (L + 1, G, 2)
  __shared__ float s_red[8];
  __shared__ float s_glam[64];
  const int tid = threadIdx.x;
  const int g = blockIdx.x, G = gridDim.x, M = gs;
  gt_partial += (size_t)g * gs;
  grad_rho_partial += (size_t)g * gs * kNRho;
  glam_partial += (size_t)g * gs;
  p += (size_t)g * kNParam;
  grad += (size_t)g * kNParam;
  {
    float v = 0.f;
    for (int i = tid; i < M; i += kThreads) v += gt_partial[i];
    v = block_sum(v, s_red);
    if (tid == 0) grad[P_T] = v;
  }
  for (int q = 0; q < kNRho; ++q) {
    float v = 0.f;
    for (int i = tid; i < M; i += kThreads) v += grad_rho_partial[(size_t)i * kNRho + q];
    v = block_sum(v, s_red);
    if (tid == 0) grad[1 + q] = v;
  }
  float gl[13];
#pragma unroll
  for (int q = 0; q < 13; ++q) gl[q] = 0.f;
  for (int k0 = 0; k0 < L; k0 += 64) {
    const int kn = (L - k0) < 64 ? (L - k0) : 64;
    for (int kk = 0; kk < kn; ++kk) {
      float v = 0.f;
      for (int i = tid; i < M; i += kThreads) v += glam_partial[(size_t)(k0 + kk) * Mtot + i];
      v = block_sum(v, s_red);
      if (tid == 0) s_glam[kk] = v;
    }
    __syncthreads();
    if (tid == 0) {
      for (int kk = 0; kk < kn; ++kk) {
        const float n = lam_in[2 * ((size_t)(k0 + kk) * G + g)], lp = lam_in[2 * ((size_t)(k0 + kk) * G + g) + 1];
        float h[3], o = p[P_LB2];
#pragma unroll
        for (int u = 0; u < 3; ++u) {
          h[u] = tanhf(fmaf(p[P_LW1 + 2 * u], n, fmaf(p[P_LW1 + 2 * u + 1], lp, p[P_LB1 + u])));
          o = fmaf(p[P_LW2 + u], h[u], o);
        }
        const float sg = sigmoidf_(o);
        const float go = s_glam[kk] * sg * (1.f - sg);
#pragma unroll
        for (int u = 0; u < 3; ++u) {
          gl[6 + 3 + u] += go * h[u];  // lambda_f.2.weight
          const float ga = go * p[P_LW2 + u] * (1.f - h[u] * h[u]);
          gl[2 * u] += ga * n;       // lambda_f.0.weight[u][0]
          gl[2 * u + 1] += ga * lp;  // lambda_f.0.weight[u][1]
          gl[6 + u] += ga;           // lambda_f.0.bias
        }
        gl[12] += go;  // lambda_f.2.bias
      }
    }
    __syncthreads();
  }
  if (tid == 0) {
#pragma unroll
    for (int q = 0; q < 13; ++q) grad[P_LW1 + q] = gl[q];
  }
}
#endif

// =============================================================================================== consensus
#ifndef UGLAD_TU_NT
__global__ void consensus_partial_kernel(const float* __restrict__ theta_K, int K, int DD, float* __restrict__ absmin,
                                         float* __restrict__ signsum) {
  for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < DD; idx += gridDim.x * blockDim.x) {
    float mn = __builtin_inff(), ss = 0.f;
    for (int k = 0; k < K; ++k) {
      const float v = theta_K[(size_t)k * DD + idx];
      mn = fminf(mn, fabsf(v));
      ss += (v > 0.f) ? 1.f : ((v < 0.f) ? -1.f : 0.f);
    }
    absmin[idx] = mn;
    signsum[idx] = ss;
  }
}
#endif

#ifndef UGLAD_TU_NT
__global__ void consensus_combine_kernel(const float* __restrict__ absmin, const float* __restrict__ signsum, int DD,
                                         float* __restrict__ out) {
  for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < DD; idx += gridDim.x * blockDim.x)
    out[idx] = (signsum[idx] >= 0.f ? 1.f : -1.f) * absmin[idx];
}
#endif

// =============================================================================================== symeig (unit-test exports)
// the LDS-lean solver alone (D <= 128): what uglad_symeig runs there, so that the unit tests of the solver (degenerate,
// clustered, graded spectra) exercise the code path of the forward cell
template <int NT>
__global__ __launch_bounds__(kThreads, NT <= 4 ? 4 : 2) void symeig_lean_kernel(float* __restrict__ U, float* __restrict__ beta,
                                                                  const float* __restrict__ tri, float* __restrict__ Tws, int D) {
  constexpr int DP = NT * 32, LD = DP + 1;
  constexpr bool kGM = DP > 128;
  __shared__ __attribute__((aligned(16))) float sQ_lds[kGM ? 4 : DP * LD];
  float* sQ = kGM ? const_cast<float*>(tri) + (size_t)gridDim.x * kWsPerMatrix<DP> + (size_t)blockIdx.x * big_floats<DP>() : sQ_lds;
  __shared__ __attribute__((aligned(16))) LeanScratch<DP> ws;
  const size_t base = (size_t)blockIdx.x * D * D;
  symeig_lean<NT>(sQ, D, ws, tri + (size_t)blockIdx.x * 3 * DP, U + base, D, Tws + (size_t)blockIdx.x * NT * 1024);
  copy_out_matrix(U + base, sQ, D, LD);
  if (threadIdx.x < D) beta[(size_t)blockIdx.x * D + threadIdx.x] = ws.d[threadIdx.x];
}

#ifdef UGLAD_STAMPS
// diagnostic build only: the solver alone, phase stamps of workgroup m copied to stamps[m*64 ..]
template <int NT>
__global__ __launch_bounds__(kThreads) void symeig_stamp_kernel(float* __restrict__ U, float* __restrict__ beta,
                                                                float* __restrict__ tri, int D,
                                                                unsigned long long* __restrict__ stamps) {
  constexpr int DP = NT * 32, LD = DP + 1;
  UGLAD_BIG_BUFFERS(sA, eig_buf0_floats<DP>(), sV, DP * LD, tri)
  __shared__ __attribute__((aligned(16))) EigScratch<DP> ws;
  const int tid = threadIdx.x;
  const size_t base = (size_t)blockIdx.x * D * D;
  if (tid < 96) ws.stamp[tid] = 0;
  __syncthreads();
  UGLAD_STAMP(ws, 0);
  symeig_from_tridiagonal<NT>(sA, sV, D, ws, tri + (size_t)blockIdx.x * 3 * DP, U + base, D);
  for (int idx = tid; idx < D * D; idx += kThreads) U[base + idx] = sV[(idx / D) * LD + (idx % D)];
  if (tid < D) beta[(size_t)blockIdx.x * D + tid] = ws.d[tid];
  __syncthreads();
  if (tid < 96) stamps[(size_t)blockIdx.x * 96 + tid] = ws.stamp[tid];
}
#endif

// =============================================================================================== covariance front-end
// What fit() does to a table before the hot path: min-max normalisation of the columns
// (prepare_data.py:597-613, main.py:85), the maximum-likelihood covariance sum_n (x_n - mu)(x_n - mu)^T / N of
// sklearn.empirical_covariance (prepare_data.py:342) and -- in a second launch, once the eigenvalues are known -- the
// reference's repair of a singular matrix (prepare_data.py:347-352).  One workgroup per task: column statistics in a first
// pass over the table, then the table streams through LDS in chunks of 64 centred rows into the upper 32x32 MFMA tiles.
template <int NT>
__global__ __launch_bounds__(kThreads) void cov_kernel(const float* __restrict__ X, int N, int D, int normalize,
                                                       float* __restrict__ S_out) {
  constexpr int DP = NT * 32, LD = DP + 1, CH = 64, G = kThreads / DP;
  __shared__ __attribute__((aligned(16))) float s_x[CH * LD];
  __shared__ float s_mn[DP], s_sc[DP], s_mu[DP];
  __shared__ float s_p[3][G][DP];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const float* Xt = X + (size_t)blockIdx.x * N * D;
  float* So = S_out + (size_t)blockIdx.x * D * D;
  // ---- pass 1: min, max, sum per column (thread = column c, row group g; rows g, g + G, ...)
  {
    const int c = tid % DP, g = tid / DP;
    if (g < G) {
      float mn = 3.4e38f, mx = -3.4e38f, sm = 0.f;
      bool nan = false;
      if (c < D)
        for (int n = g; n < N; n += G) {
          const float v = Xt[(size_t)n * D + c];
          nan = nan || (v != v);
          mn = fminf(mn, v);
          mx = fmaxf(mx, v);
          sm += v;
        }
      s_p[0][g][c] = nan ? __builtin_nanf("") : mn;
      s_p[1][g][c] = mx;
      s_p[2][g][c] = sm;
    }
  }
  __syncthreads();
  if (tid < DP) {
    float mn = s_p[0][0][tid], mx = s_p[1][0][tid], sm = s_p[2][0][tid];
    for (int g = 1; g < G; ++g) {
      const float a = s_p[0][g][tid];
      mn = (a != a || mn != mn) ? __builtin_nanf("") : fminf(mn, a);
      mx = fmaxf(mx, s_p[1][g][tid]);
      sm += s_p[2][g][tid];
    }
    const float mean = sm / (float)N;
    if (normalize == 1) {  // (x - min) / (max - min): a constant column gives 0/0 = NaN, as in the reference
      const float sc = 1.0f / (mx - mn);
      s_mn[tid] = mn;
      s_sc[tid] = sc;
      s_mu[tid] = (mean - mn) * sc;
    } else {
      s_mn[tid] = 0.f;
      s_sc[tid] = 1.f;
      s_mu[tid] = mean;
    }
  }
  __syncthreads();
  // ---- pass 2: S = sum over chunks of Xc^T Xc on the upper tiles
  using T = Tiles<NT, true>;
  f32x16 acc[T::kPerWave];
#pragma unroll
  for (int n = 0; n < T::kPerWave; ++n)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[n][e] = 0.f;
  for (int r0 = 0; r0 < N; r0 += CH) {
    for (int idx = tid; idx < CH * DP; idx += kThreads) {
      const int r = idx / DP, c = idx - r * DP;
      float v = 0.f;
      if (r0 + r < N && c < D) v = (Xt[(size_t)(r0 + r) * D + c] - s_mn[c]) * s_sc[c] - s_mu[c];
      s_x[r * LD + c] = v;
    }
    __syncthreads();
#pragma unroll
    for (int n = 0; n < T::kPerWave; ++n) {
      const int t = w + kWaves * n;
      if (t < T::kCount) {
        int I, J;
        T::ij(t, I, J);
        mfma_tile(s_x + I * 32, 1, LD, s_x + J * 32, LD, 1, CH, acc[n]);
      }
    }
    __syncthreads();
  }
  const float inv_n = 1.0f / (float)N;
#pragma unroll
  for (int n = 0; n < T::kPerWave; ++n) {
    const int t = w + kWaves * n;
    if (t < T::kCount) {
      int I, J;
      T::ij(t, I, J);
      const int j = J * 32 + (lane & 31);
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int i = I * 32 + acc_row(e, lane);
        if (i <= j && j < D) {
          const float v = acc[n][e] * inv_n;
          So[i * D + j] = v;
          if (i != j) So[j * D + i] = v;
        }
      }
    }
  }
}

// S += (offset - min eig) I where the smallest eigenvalue is <= 1e-6 (beta ascending: beta[0] is the smallest)
#ifndef UGLAD_TU_NT
__global__ void cov_repair_kernel(float* __restrict__ S, const float* __restrict__ beta, int D, float offset) {
  const float mn = beta[(size_t)blockIdx.x * D];
  if (mn <= 1e-6f) {
    float* So = S + (size_t)blockIdx.x * D * D;
    for (int i = threadIdx.x; i < D; i += blockDim.x) So[i * D + i] += offset - mn;
  }
}
#endif

// =============================================================================================== after the path
// ---- N3: conditional Gaussian / MAP estimate given observed coordinates (main.py:1176-1260).  With the precision matrix
// partitioned into unobserved (u) and observed (o) coordinates the reference computes  mean_u - L_uu^-1 L_uo (x_o - mean_o)
// (scipy.linalg.solve), the conditional covariance L_uu^-1 and the density at the MAP point.  Here L_uu stays IN PLACE: the
// masked matrix A (A_ij = P_ij for i, j both unobserved, delta_ij otherwise) has L_uu^-1 as the (u, u) block of its inverse and
// the identity elsewhere, so no gather / scatter is needed and the path's own eigensolver does the solve.
#ifndef UGLAD_TU_NT
__global__ void map_prepare_kernel(const float* __restrict__ P, const float* __restrict__ observed, float* __restrict__ A, int D,
                                   size_t total) {
  const size_t dd = (size_t)D * D;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
    const size_t m = idx / dd;
    const int r = (int)(idx - m * dd);
    const int i = r / D, j = r - i * D;
    const bool keep = observed[m * D + i] == 0.f && observed[m * D + j] == 0.f;
    // (the upper-triangle value on both sides: the solver assumes exact symmetry)
    A[idx] = keep ? P[m * dd + (i <= j ? (size_t)i * D + j : (size_t)j * D + i)] : ((i == j) ? 1.f : 0.f);
  }
}
#endif

template <int NT>
__global__ __launch_bounds__(kThreads) void map_solve_kernel(const float* __restrict__ P, const float* __restrict__ mean,
                                                             const float* __restrict__ observed,
                                                             const float* __restrict__ values, const float* __restrict__ A,
                                                             float* __restrict__ full_mean, float* __restrict__ cond_cov,
                                                             float* __restrict__ log_pdf, float* __restrict__ tri, int D,
                                                             int clip01) {
  constexpr int DP = NT * 32, LD = DP + 1;
  UGLAD_BIG_BUFFERS(sA, eig_buf0_floats<DP>(), sV, DP * LD, tri)
  __shared__ __attribute__((aligned(16))) EigScratch<DP> ws;
  __shared__ float s_f[DP], s_r[DP], s_t[DP], s_y[DP], s_red[8];
  const int tid = threadIdx.x;
  const size_t base = (size_t)blockIdx.x * D * D;
  const float* Pm = P + base;
  const float* Am = A + base;
  const float* mu = mean + (size_t)blockIdx.x * D;
  const float* ob = observed + (size_t)blockIdx.x * D;
  const float* xv = values + (size_t)blockIdx.x * D;
  // right-hand side r_u = L_uo (x_o - mean_o), zero on the observed coordinates
  if (tid < DP) {
    float r = 0.f;
    if (tid < D && ob[tid] == 0.f) {
      for (int j = 0; j < D; ++j)
        if (ob[j] != 0.f) r = fmaf(Pm[tid <= j ? tid * D + j : j * D + tid], xv[j] - mu[j], r);
    }
    s_r[tid] = r;
  }
  symeig_from_tridiagonal<NT>(sA, sV, D, ws, tri + (size_t)blockIdx.x * 3 * DP, cond_cov + base, D);
  float lad = 0.f, bad = 0.f, nu = 0.f;
  if (tid < DP) {
    float f = 0.f;
    if (tid < D) {
      const float be = ws.d[tid];
      f = 1.0f / be;
      lad = logf(be);  // (NaN for a negative eigenvalue: L_uu not positive definite)
      bad = (be > 0.f) ? 0.f : 1.f;
      nu = (ob[tid] == 0.f) ? 1.f : 0.f;
    }
    s_f[tid] = f;
  }
  lad = block_sum(lad, s_red);
  bad = block_sum(bad, s_red);
  nu = block_sum(nu, s_red);
  // y = A^-1 r = V diag(1/beta) V^T r, then one step of iterative refinement y += A^-1 (r - A y) (A from global memory)
  auto apply_inverse = [&](const float* __restrict__ rhs, float* __restrict__ dst, bool accumulate) {
    if (tid < DP) {
      float t = 0.f;
      for (int i = 0; i < D; ++i) t = fmaf(sV[i * LD + tid], rhs[i], t);
      s_t[tid] = t * s_f[tid];
    }
    __syncthreads();
    if (tid < DP) {
      float y = 0.f;
      if (tid < D)
        for (int k = 0; k < D; ++k) y = fmaf(sV[tid * LD + k], s_t[k], y);
      dst[tid] = accumulate ? dst[tid] + y : y;
    }
    __syncthreads();
  };
  apply_inverse(s_r, s_y, false);
  if (tid < DP) {
    float res = 0.f;
    if (tid < D) {
      res = s_r[tid];
      for (int j = 0; j < D; ++j) res = fmaf(-Am[tid * D + j], s_y[j], res);
    }
    sA[tid] = res;  // (sA is free between the solver and spectral_to_global)
  }
  __syncthreads();
  apply_inverse(sA, s_y, true);
  if (tid < D) {
    float v = (ob[tid] != 0.f) ? xv[tid] : mu[tid] - s_y[tid];
    if (clip01) v = fminf(fmaxf(v, 0.f), 1.f);
    full_mean[(size_t)blockIdx.x * D + tid] = v;
  }
  if (tid == 0 && log_pdf)
    log_pdf[blockIdx.x] = (bad > 0.f) ? __builtin_nanf("") : fmaf(-0.5f * nu, 1.8378770664093453f, 0.5f * lad);
  __syncthreads();
  spectral_to_global<NT>(sA, sV, s_f, cond_cov + base, D, Am, 0.f);  // A^-1: L_uu^-1 on the (u, u) block, identity elsewhere
}

// ---- N4: partial correlations (main.py:796-821): rho_ij = -p_ij / sqrt(p_ii p_jj) from the UPPER triangle, mirrored, 1 on the diagonal
#ifndef UGLAD_TU_NT
__global__ void partial_corr_kernel(const float* __restrict__ P, float* __restrict__ rho, int D, size_t total) {
  const size_t dd = (size_t)D * D;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
    const size_t m = idx / dd;
    const int r = (int)(idx - m * dd);
    const int i = r / D, j = r - i * D;
    const float* Pm = P + m * dd;
    const int a = i < j ? i : j, b = i < j ? j : i;
    rho[idx] = (i == j) ? 1.f : -Pm[(size_t)a * D + b] / sqrtf(Pm[(size_t)a * D + a] * Pm[(size_t)b * D + b]);
  }
}
#endif

// ---- N4: support-recovery metrics of report_metrics_all (utils/metrics.py:25-108) for one (true, predicted) pair per
// workgroup.  Edges = strict upper triangle; an edge is predicted where the entry is non-zero; scores for the ranking metrics
// are |entry|.  All counting is integer (exact, order-independent): ROC-AUC is the Mann-Whitney statistic with ties at 1/2
// (the trapezoid of sklearn.metrics.roc_curve), average precision is (1/T) sum over true edges of precision at that edge's
// score (sklearn.metrics.average_precision_score: thresholds are the distinct scores).  out[0..10] (double): FDR, TPR, FPR,
// SHD, nnzTrue, nnzPred, precision, recall, Fbeta, aupr, auc -- unrounded (the host rounds to 3 decimals as the reference does).
template <int NT>
__global__ __launch_bounds__(kThreads) void support_metrics_kernel(const float* __restrict__ true_theta,
                                                                   const float* __restrict__ pred_theta,
                                                                   double* __restrict__ out, int D, int beta) {
  constexpr int DP = NT * 32, EMAX = DP * (DP - 1) / 2;
  __shared__ float s_score[EMAX];            // |pred| of edge e
  __shared__ int s_true[EMAX / 32 + 1];       // bit e: the edge exists in the true graph
  __shared__ long long s_cnt[kThreads];
  __shared__ double s_dbl[kThreads];
  const int tid = threadIdx.x;
  const size_t base = (size_t)blockIdx.x * D * D;
  const int E = D * (D - 1) / 2;
  for (int w = tid; w < EMAX / 32 + 1; w += kThreads) s_true[w] = 0;
  __syncthreads();
  for (int idx = tid; idx < D * D; idx += kThreads) {
    const int i = idx / D, j = idx - i * D;
    if (i < j) {
      const int e = i * D - (i * (i + 1)) / 2 + (j - i - 1);
      s_score[e] = fabsf(pred_theta[base + idx]);
      if (true_theta[base + idx] != 0.f) atomicOr(&s_true[e >> 5], (int)(1u << (e & 31)));
    }
  }
  __syncthreads();
  auto is_true = [&](int e) { return (((unsigned)s_true[e >> 5]) >> (e & 31)) & 1u; };
  // reduce a per-thread integer over the workgroup, in index order
  auto total = [&](long long v) {
    s_cnt[tid] = v;
    __syncthreads();
    long long t = 0;
    if (tid == 0)
      for (int q = 0; q < kThreads; ++q) t += s_cnt[q];
    __syncthreads();
    return t;  // valid on thread 0
  };
  long long tp = 0, np_ = 0, nt = 0;
  for (int e = tid; e < E; e += kThreads) {
    const bool t = is_true(e), p = s_score[e] != 0.f;
    tp += (t && p) ? 1 : 0;
    np_ += p ? 1 : 0;
    nt += t ? 1 : 0;
  }
  const long long TP = total(tp), Pn = total(np_), Tn = total(nt);
  // ranking statistics: one true edge per thread and pass, all E scores swept from LDS (same address on every lane: broadcast)
  long long mw2 = 0;  // sum over true edges of 2 #(false edges with a smaller score) + #(false edges with an equal score)
  double ap = 0.0;
  for (int e = tid; e < E; e += kThreads) {
    if (!is_true(e)) continue;
    const float se = s_score[e];
    int lt = 0, eq = 0, ge_all = 0, ge_pos = 0;
    for (int w0 = 0; w0 < E; w0 += 32) {
      const unsigned bits = (unsigned)s_true[w0 >> 5];
      const int lim = (E - w0) < 32 ? (E - w0) : 32;
      for (int b = 0; b < lim; ++b) {
        const float sf = s_score[w0 + b];
        const bool t = (bits >> b) & 1u;
        lt += (!t && sf < se) ? 1 : 0;
        eq += (!t && sf == se) ? 1 : 0;
        ge_all += (sf >= se) ? 1 : 0;
        ge_pos += (t && sf >= se) ? 1 : 0;
      }
    }
    mw2 += 2LL * lt + eq;
    ap += (double)ge_pos / (double)ge_all;
  }
  const long long MW2 = total(mw2);
  s_dbl[tid] = ap;
  __syncthreads();
  if (tid == 0) {
    double AP = 0.0;
    for (int q = 0; q < kThreads; ++q) AP += s_dbl[q];
    const double dTP = (double)TP, dP = (double)Pn, dT = (double)Tn, dF = (double)E - dT;
    const double FP = dP - dTP, FN = dT - dTP;
    const double b2 = (double)beta * (double)beta;
    double* o = out + (size_t)blockIdx.x * 11;
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

// the round-1 Jacobi solver, kept as an independent on-device cross-check of the divide & conquer path
template <int NT>
__global__ __launch_bounds__(kThreads) void symeig_jacobi_kernel(const float* __restrict__ A, float* __restrict__ U,
                                                                 float* __restrict__ beta, int D) {
  constexpr int DP = NT * 32, LD = DP + 1;
  __shared__ float sA[DP * LD];
  __shared__ float sV[DP * LD];
  __shared__ float s_t[DP / 2], s_s[DP / 2], s_h[DP / 2], s_red[8];
  __shared__ int s_flag;
  const int tid = threadIdx.x;
  const size_t base = (size_t)blockIdx.x * D * D;
  for (int idx = tid; idx < DP * DP; idx += kThreads) {
    const int i = idx / DP, j = idx - i * DP;
    float v = 0.f;
    if (i < D && j < D) v = A[base + (i < j ? i * D + j : j * D + i)];
    sA[i * LD + j] = v;
    sV[i * LD + j] = (i == j) ? 1.f : 0.f;
  }
  __syncthreads();
  jacobi_eig<DP>(sA, sV, s_t, s_s, s_h, s_red, &s_flag);
  for (int idx = tid; idx < D * D; idx += kThreads) {
    const int i = idx / D, k = idx - i * D;
    U[base + idx] = sV[i * LD + k];
  }
  if (tid < D) beta[(size_t)blockIdx.x * D + tid] = sA[tid * LD + tid];
}

// ---- one translation unit per NT (the build of __graft_entry__.py): compiled with -DUGLAD_TU_NT=k this file emits ONLY the
// kernels templated on NT = k (explicit instantiations; the C ABI below is skipped), compiled with -DUGLAD_TU_HOST it emits
// everything else and merely declares those instantiations.  The units compile in parallel and link into one library.
// Without either macro (emulator and sanitizer builds) the file is one self-contained unit as before.
#define UGLAD_PER_NT_KERNELS(X, NT)                                                                                             \
  X void tridiag_kernel<NT, kThreads>(const float*, const float*, const float*, float*, float*, int, int, const int*);                  \
  X void cell_bwd_kernel<NT>(const float*, const float*, const float*, const float*, const float*, const float*, const float*, \
                             const float*, float*, float*, float*, float*, int, int, int, int, int);                            \
  X void init_inverse_kernel<NT>(const float*, const float*, float*, float*, int, int, const int*);                            \
  X void init_bwd_kernel<NT>(const float*, const float*, float*, float*, int);                                                 \
  X void loss_fwd_kernel<NT>(const float*, const float*, int, const float*, float*, float*, float*, int, const int*);          \
  X void cov_kernel<NT>(const float*, int, int, int, float*);                                                                  \
  X void map_solve_kernel<NT>(const float*, const float*, const float*, const float*, const float*, float*, float*, float*,   \
                              float*, int, int);                                                                                \
  X void support_metrics_kernel<NT>(const float*, const float*, double*, int, int);                                            \
  X void symeig_lean_kernel<NT>(float*, float*, const float*, float*, int);                                                    \
  X void cell_fwd_lean_kernel<NT>(const float*, const float*, const float*, const float*, float*, float*, float*, float*,     \
                                  float*, float*, const float*, float*, int, int, int, int, LamStep);
// the dL/dS variants (uglad_glad_backward_wrt_s) in translation units of their own (-DUGLAD_TU_GS): instantiated next to the kernels above
// they changed how the compiler treated cell_bwd_kernel<3> (80 instead of 78 SGPR spills, scripts/kernel_meta.py)
#define UGLAD_PER_NT_GS(X, NT)                                                                                                  \
  X void cell_bwd_gs_kernel<NT>(const float*, const float*, const float*, const float*, const float*, const float*, const float*, \
                                const float*, float*, float*, float*, float*, int, int, int, int, int, float*);                  \
  X void init_bwd_gs_kernel<NT>(const float*, const float*, float*, float*, int);
#define UGLAD_PER_NT_SMALL(X, NT)                                                                                       \
  X void symeig_jacobi_kernel<NT>(const float*, float*, float*, int);                                                  \
  X void chol_init_kernel<NT>(const float*, const float*, float*, int*, int, int);                                     \
  X void chol_loss_kernel<NT>(const float*, const float*, int, const float*, float*, float*, int*, int);
// D <= 96: the tridiagonalisation with 16 column groups as at D = 128 (128 NT threads) instead of 512 threads -- with 512 the chain wave gathers
// 512 / (DP / 4) partial sums per row, 64 at DP = 32, most of them zeros (profiles/r04_tridiag_small.txt)
#define UGLAD_PER_NT_TRISMALL(X, NT) \
  X void tridiag_kernel<NT, 128 * NT>(const float*, const float*, const float*, float*, float*, int, int, const int*);
// D <= 32: one wave per matrix, the matrix in its registers (tridiag_wave.h)
#define UGLAD_PER_NT_TRIWAVE(X, NT) X void tridiag_wave_kernel<NT>(const float*, const float*, const float*, float*, float*, int, int, const int*);
#define UGLAD_PER_NT_BIG(X, NT)                                                                             \
  X void tridiag_kernel<NT, 1024>(const float*, const float*, const float*, float*, float*, int, int, const int*); \
  X void cell_fwd_back_kernel<NT>(const float*, float*, const float*, float*, float*, int, int);
#ifdef UGLAD_STAMPS
#define UGLAD_PER_NT_DIAG(X, NT) X void symeig_stamp_kernel<NT>(float*, float*, float*, int, unsigned long long*);
#else
#define UGLAD_PER_NT_DIAG(X, NT)
#endif
#if defined(UGLAD_TU_NT) && defined(UGLAD_DEV_ONLY_LEAN)
// development (scripts/spill_check.sh): the forward cell's second stage alone, to read its register allocation in seconds
template __global__ void cell_fwd_lean_kernel<UGLAD_TU_NT>(const float*, const float*, const float*, const float*, float*, float*, float*,
                                                          float*, float*, float*, const float*, float*, int, int, int, int, LamStep);
#elif defined(UGLAD_TU_NT) && defined(UGLAD_DEV_ONLY_TRIDIAG)
template __global__ void tridiag_kernel<UGLAD_TU_NT, kThreads>(const float*, const float*, const float*, float*, float*, int, int, const int*);
#elif defined(UGLAD_TU_NT) && defined(UGLAD_DEV_ONLY_BWD)
template __global__ void cell_bwd_kernel<UGLAD_TU_NT>(const float*, const float*, const float*, const float*, const float*, const float*,
                                                     const float*, const float*, float*, float*, float*, float*, int, int, int, int, int);
#elif defined(UGLAD_TU_NT) && defined(UGLAD_DEV_ONLY_TRIWAVE)
UGLAD_PER_NT_TRIWAVE(template __global__, UGLAD_TU_NT)
#elif defined(UGLAD_TU_NT) && defined(UGLAD_DEV_ONLY_CHOL)
UGLAD_PER_NT_SMALL(template __global__, UGLAD_TU_NT)
#elif defined(UGLAD_TU_NT) && defined(UGLAD_TU_GS)
UGLAD_PER_NT_GS(template __global__, UGLAD_TU_NT)
#elif defined(UGLAD_TU_NT)
UGLAD_PER_NT_KERNELS(template __global__, UGLAD_TU_NT)
UGLAD_PER_NT_DIAG(template __global__, UGLAD_TU_NT)
#if UGLAD_TU_NT <= 4
UGLAD_PER_NT_SMALL(template __global__, UGLAD_TU_NT)
#if UGLAD_TU_NT <= 3
UGLAD_PER_NT_TRISMALL(template __global__, UGLAD_TU_NT)
#endif
#if UGLAD_TU_NT == 1
UGLAD_PER_NT_TRIWAVE(template __global__, UGLAD_TU_NT)
#endif
#else
UGLAD_PER_NT_BIG(template __global__, UGLAD_TU_NT)
#endif
#elif defined(UGLAD_TU_HOST)
#define UGLAD_DECLARE_NT(NT) UGLAD_PER_NT_KERNELS(extern template __global__, NT) UGLAD_PER_NT_DIAG(extern template __global__, NT) \
  UGLAD_PER_NT_GS(extern template __global__, NT)
UGLAD_DECLARE_NT(1) UGLAD_DECLARE_NT(2) UGLAD_DECLARE_NT(3) UGLAD_DECLARE_NT(4)
UGLAD_PER_NT_SMALL(extern template __global__, 1) UGLAD_PER_NT_SMALL(extern template __global__, 2)
UGLAD_PER_NT_SMALL(extern template __global__, 3) UGLAD_PER_NT_SMALL(extern template __global__, 4)
UGLAD_PER_NT_TRISMALL(extern template __global__, 1) UGLAD_PER_NT_TRISMALL(extern template __global__, 2) UGLAD_PER_NT_TRISMALL(extern template __global__, 3)
UGLAD_PER_NT_TRIWAVE(extern template __global__, 1)
UGLAD_DECLARE_NT(5) UGLAD_DECLARE_NT(6) UGLAD_DECLARE_NT(7) UGLAD_DECLARE_NT(8)
UGLAD_PER_NT_BIG(extern template __global__, 5) UGLAD_PER_NT_BIG(extern template __global__, 6)
UGLAD_PER_NT_BIG(extern template __global__, 7) UGLAD_PER_NT_BIG(extern template __global__, 8)
#endif

}  // namespace uglad

#ifndef UGLAD_TU_NT
// =============================================================================================== the host layer (no device code)
#include "host_route.h"
#include "host_launch.h"
#include "host_api.h"
#include "host_rccl.h"
#include "host_extra.h"
#endif  // !UGLAD_TU_NT
